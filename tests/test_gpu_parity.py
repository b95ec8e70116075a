"""GPU parity tests: the HIP path (through the C ABI of include/sift_hip.h) against the CPU oracle
on the same seeded inputs.  Bit-exact for every float image, index and flag; descriptors are also
required bit-exact (north_star tolerance: 1e-4 L2 — asserted as the fallback bound).
"""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from golden_util import read_pgm
from sift_amd import _lib
from sift_amd.sift import Context, PreconditionViolation, Sift, gauss_taps
from sift_amd.synthetic import synth_frame

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-4  # L2 per descriptor, BASELINE.json north_star


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what, report=None):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    neq = bits(a) != bits(b)
    # NaN payloads: treat NaN == NaN
    neq &= ~(np.isnan(a) & np.isnan(b))
    n = int(neq.sum())
    if n:
        idx = np.argwhere(neq)[:5]
        detail = [(tuple(int(v) for v in i), float(a[tuple(i)]), float(b[tuple(i)])) for i in idx]
        msg = f"{what}: {n}/{a.size} values differ; first: {detail}; max abs diff {float(np.nanmax(np.abs(a - b)))}"
        if report is not None:
            report.append(msg)
        raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------
# operator-level known-answer tests
# ------------------------------------------------------------------------------------------------
CONVOLVE_SIGMAS = [1.0, 1.6, 2.2627418, 3.2, 4.5254836, 6.4, 9.050967, 12.8, 0.3, 0.0]


def convolve_cases(ctx, sigma, what):
    for (w, h, seed) in [(200, 150, 3), (67, 131, 4), (64, 64, 5)]:
        img = synth_frame(w, h, seed)
        r, _ = O.gauss_taps(sigma)
        if min(w, h) < r + 1:
            with pytest.raises(PreconditionViolation):
                ctx.convolve_with_gauss(img, sigma)
            continue
        assert_bits_equal(ctx.convolve_with_gauss(img, sigma), O.convolve(img, sigma), f"blur s={sigma} {w}x{h} {what}")


@pytest.mark.parametrize("sigma", CONVOLVE_SIGMAS)
def test_convolve_with_gauss(ctx, sigma):
    """alg::convolveWithGauss (algorithms.cpp:10-22) on ragged shapes: the LDS-tiled kernel for radii 1 .. 32, the two-pass
    kernels beyond (sigma 12.8: radius 38) and for radius 0 (sigma 0); the two-pass form forced for every radius is one of
    tests/diag_fallbacks.py's cases."""
    convolve_cases(ctx, sigma, "default path")


@pytest.mark.parametrize("sigmas", [(0.3, 1.0), (1.6, 2.0), (2.2627418, 3.2), (4.0, 4.5254836)], ids=["r1-3", "r5-6", "r7-10", "r12-14"])
def test_convolve_with_gauss_streaming(ctx, sigmas):
    """The streaming blur (the form the bench workload runs, radius <= 14) forced onto small single frames: ragged
    strips, one-chunk and many-chunk launches, widths that only the 2-columns-per-lane form accepts."""
    ctx.set_option("stream_min_waves", 1)
    try:
        for sigma in sigmas:
            for (w, h, seed) in [(200, 150, 3), (64, 64, 5), (260, 301, 6), (1028, 97, 7), (130, 515, 8), (516, 40, 9)]:
                img = synth_frame(w, h, seed)
                r, _ = O.gauss_taps(sigma)
                if min(w, h) < r + 1:
                    continue
                assert_bits_equal(ctx.convolve_with_gauss(img, sigma), O.convolve(img, sigma), f"streaming blur s={sigma} {w}x{h}")
    finally:
        ctx.set_option("stream_min_waves", 0)


def test_gauss_taps_match_oracle():
    for sigma in [0.0, 0.2, 1.0, 1.6, 2.2627418, 3.2, 4.5254836, 6.4, 9.050967, 12.8, 18.101934, 50.0]:
        r1, t1 = gauss_taps(sigma)
        r2, t2 = O.gauss_taps(sigma)
        assert r1 == r2
        assert t1.tobytes() == t2.tobytes()


def test_blur_precondition_messages(ctx):
    img = synth_frame(40, 12, 1)
    with pytest.raises(PreconditionViolation, match=r"separableConvolveY\(\): kernel longer than line"):
        ctx.convolve_with_gauss(img, 4.5254836)  # r = 14 > 11
    with pytest.raises(PreconditionViolation, match=r"separableConvolveX\(\): kernel longer than line"):
        ctx.convolve_with_gauss(np.ascontiguousarray(img.T), 4.5254836)
    with pytest.raises(PreconditionViolation, match="Standard deviation"):
        ctx.convolve_with_gauss(img, -1.0)


def test_resample(ctx):
    for (h, w) in [(135, 240), (150, 201), (64, 64), (37, 90)]:
        img = synth_frame(w, h, 7)
        assert_bits_equal(ctx.reduce_to_next_level(img, 1.6), O.resample(img, 1.6, 0), f"reduce {w}x{h}")
        assert_bits_equal(ctx.increase_to_next_level(img, 1.0), O.resample(img, 1.0, 1), f"increase {w}x{h}")


def test_dog_and_gradient(ctx):
    a = synth_frame(173, 91, 11)
    b = O.convolve(a, 1.6)
    out = np.empty_like(a)
    O.lib().oracle_dog(a, b, a.shape[1], a.shape[0], out)
    assert_bits_equal(ctx.dog(a, b), out, "dog")
    mag, ori = np.empty_like(b), np.empty_like(b)
    O.lib().oracle_gradient(b, b.shape[1], b.shape[0], mag, ori)
    gm, go = ctx.gradient(b)
    assert_bits_equal(gm, mag, "gradient magnitude")
    assert_bits_equal(go, ori, "gradient orientation")
    # harsher inputs for atan2f / sqrt: random floats incl. tiny and huge differences
    rng = np.random.default_rng(5)
    c = (rng.standard_normal((64, 96)) * 10.0 ** rng.integers(-6, 6, (64, 96))).astype(np.float32)
    O.lib().oracle_gradient(c, c.shape[1], c.shape[0], mag := np.empty_like(c), ori := np.empty_like(c))
    gm, go = ctx.gradient(c)
    assert_bits_equal(gm, mag, "gradient magnitude (wide range)")
    assert_bits_equal(go, ori, "gradient orientation (wide range)")
    # round 6: the magnitude takes one Newton round on the hardware's reciprocal-square-root estimate and the correctly
    # rounded routine only near a float rounding boundary (sift_amd/csrc/grad_math.h).  A lattice of pixels whose (dx, dy)
    # put sqrt(dx^2 + dy^2) within ~2^-47 of the midpoint of two floats - just above, just below, and as close as float
    # inputs get - plus random pairs in between; every pixel against the oracle, magnitudes also against numpy's sqrt.
    from test_host_math import midpoint_pairs
    rng = np.random.default_rng(6)
    side = 1024
    k = (side // 4) ** 2
    d = np.zeros((side, side), np.float32)
    dxs, dys = [], []
    for steps in (0, 1):
        dxa, dya, _ = midpoint_pairs(rng, k // 8, steps)
        for bump in (0, 1, -1):
            dxs.append(dxa)
            dys.append((dya.view(np.int32) + bump).view(np.float32))
    rest = k - sum(a.size for a in dxs)
    dxs.append((rng.standard_normal(rest) * 10.0 ** rng.integers(-5, 3, rest)).astype(np.float32))
    dys.append((rng.standard_normal(rest) * 10.0 ** rng.integers(-5, 3, rest)).astype(np.float32))
    dxs, dys = np.concatenate(dxs).reshape(side // 4, side // 4), np.concatenate(dys).reshape(side // 4, side // 4)
    d[1::4, 2::4] = dxs          # right neighbour of pixel (4i+1, 4j+1); its left, up neighbours stay 0
    d[2::4, 1::4] = dys          # down neighbour
    O.lib().oracle_gradient(d, side, side, mag := np.empty_like(d), ori := np.empty_like(d))
    gm, go = ctx.gradient(d)
    assert_bits_equal(gm, mag, "gradient magnitude (pairs at float rounding boundaries)")
    assert_bits_equal(go, ori, "gradient orientation (pairs at float rounding boundaries)")
    want = np.sqrt(dxs.astype(np.float64) ** 2 + dys.astype(np.float64) ** 2).astype(np.float32)
    assert_bits_equal(gm[1::4, 1::4], want, "gradient magnitude against numpy's correctly rounded square root")


def test_edge_responses_and_parabola(ctx):
    img = synth_frame(160, 120, 21)
    g = [O.convolve(img, s) for s in (1.6, 2.2627418, 3.2, 4.5254836)]
    d = []
    for i in range(3):
        out = np.empty_like(img)
        O.lib().oracle_dog(g[i], g[i + 1], img.shape[1], img.shape[0], out)
        d.append(out)
    ys, xs = np.mgrid[1:119, 1:159]
    xs, ys = xs.ravel().astype(np.uint16), ys.ravel().astype(np.uint16)
    got = ctx.edge_responses(d[0], d[1], d[2], xs, ys)
    want = np.array([O.lib().oracle_edge_filtered(d[0], d[1], d[2], 160, 120, int(x), int(y)) for x, y in zip(xs, ys)], np.uint8)
    assert (got == want).all(), f"edge filter flags differ at {int((got != want).sum())} of {got.size} points"
    assert 0 < want.sum() < want.size

    rng = np.random.default_rng(2)
    m = 5000
    i = rng.integers(0, 36, m)
    lnx = np.where(i == 0, 355, (i - 1) * 10 + 5).astype(np.uint16)
    rnx = np.where(i == 35, 5, (i + 1) * 10 + 5).astype(np.uint16)
    px = (i * 10 + 5).astype(np.uint16)
    hs = (rng.random((3, m)) * 10.0 ** rng.integers(-3, 6, (3, m))).astype(np.float32)
    hs[0, ::3] = 0
    hs[2, ::3] = 0
    got = ctx.vertex_parabola(lnx, hs[0], px, hs[1], rnx, hs[2])
    want = np.array([O.lib().oracle_vertex_parabola(int(a), float(b), int(c), float(dd), int(e), float(f))
                     for a, b, c, dd, e, f in zip(lnx, hs[0], px, hs[1], rnx, hs[2])], np.float32)
    assert_bits_equal(got, want, "vertexParabola")


# ------------------------------------------------------------------------------------------------
# whole pipeline, stage by stage
# ------------------------------------------------------------------------------------------------
CASES = [
    # name, w, h, seed, dogs, octaves, subpixel
    ("synthetic 160x120 2oct", 160, 120, 1, 3, 2, False),
    ("synthetic 640x480 4x3 (config 2)", 640, 480, 1, 3, 4, False),
    ("synthetic 333x257 3oct odd sizes", 333, 257, 9, 3, 3, False),
    ("synthetic 320x240 subpixel", 320, 240, 5, 3, 3, True),
    ("synthetic 400x300 4 dogs", 400, 300, 6, 4, 2, False),
    ("synthetic 322x250 widths 2 mod 4 / odd", 322, 250, 12, 3, 3, False),   # streaming blur with 2 columns per lane, unfused scan, scalar gradient
    ("synthetic 1024x768 4x3", 1024, 768, 13, 3, 4, False),
]


def compare_gradient_maps(ctx, run, image, dogs, octaves, name, rep=None):
    """The gradient maps of every level: sift_hip_level_copy's `magnitude` / `orientation` against the oracle's.

    The two sides keep a level's maps in different states.  The reference's descriptor stage adds to its maps in place, keypoint
    after keypoint (sift.cpp:80-92), and the oracle's `level` serves that FINAL state; the library recomputes those additions per
    keypoint and leaves the maps as the gradient pass wrote them (kernels_desc.hip).  So a map is required bit-identical
      - to the oracle's final map at every pixel outside the 16x16 windows of the final keypoints that select the level - where
        final and first state are the same thing (so those windows are all the oracle's map may have changed in) -, and
      - at every pixel to the oracle's own gradient functions (oracle_gradient: sift.cpp:130-160 for one level) applied to the
        ORACLE's Gaussian level.
    Which levels have maps: the reference forms them for every level; the oracle forms a level's when a keypoint first selects it,
    the library those that the plan's scanned DoG levels select (its restatement of _findNearestGaussian, for any image).  A
    level the oracle has and the library lacks fails.  A level only the library has - no keypoint of THIS image selects it - is
    held to the second requirement.  -> (levels both have, levels only the library has)."""
    import scale_ref
    final = run.points("final")[0]
    gauss = [[run.scale("gaussian", o, j) for j in range(dogs + 1)] for o in range(octaves)]
    nearest = {oi: scale_ref.find_nearest_gaussian(gauss, run.scale("dog", *oi)) for oi in set(zip(final["octave"].tolist(), final["index"].tolist()))}
    selects = [nearest[oi] for oi in zip(final["octave"].tolist(), final["index"].tolist())]
    both, library_only = [], []
    for o in range(octaves):
        for j in range(dogs + 1):
            got = {kind: ctx.level(kind, o, j, image) for kind in ("magnitude", "orientation")}
            want = {kind: run.level(kind, o, j) for kind in ("magnitude", "orientation")}
            assert (got["magnitude"] is None) == (got["orientation"] is None) and (want["magnitude"] is None) == (want["orientation"] is None)
            assert want["magnitude"] is None or got["magnitude"] is not None, \
                f"{name}: level ({o},{j}) img{image}: the oracle has gradient maps (a keypoint selects the level), the library has none"
            if got["magnitude"] is None:
                continue
            (both if want["magnitude"] is not None else library_only).append((o, j))
            g = run.level("gaussian", o, j)
            h, w = g.shape
            first = {"magnitude": np.empty_like(g), "orientation": np.empty_like(g)}
            O.lib().oracle_gradient(g, w, h, first["magnitude"], first["orientation"])
            covered = np.zeros((h, w), bool)
            for x, y, sel in zip(final["x"].tolist(), final["y"].tolist(), selects):
                if sel == (o, j):
                    covered[max(y - 8, 0):y + 8, max(x - 8, 0):x + 8] = True
            for kind in ("magnitude", "orientation"):
                what = f"{name}: {kind}({o},{j}) img{image}"
                assert got[kind].shape == (h, w), f"{what}: shape {got[kind].shape} vs oracle {(h, w)}"
                if want[kind] is not None:
                    assert_bits_equal(np.where(covered, 0, got[kind]), np.where(covered, 0, want[kind]), what + " outside the keypoints' windows")
                assert_bits_equal(got[kind], first[kind], what + " against the oracle's gradient of its own level")
    if rep is not None:
        rep["gradient_levels"] = [list(l) for l in both]
        rep["gradient_levels_unselected"] = [list(l) for l in library_only]
    return both, library_only


def compare_image(ctx, run, image, dogs, octaves, subpixel, name, rep):
    """Image `image` of the batch the context holds against one oracle run of that image: the replaced image (subpixel), every
    Gaussian and DoG level, the gradient maps of every level that has them and every stage list; the stage sizes go into `rep`."""
    if subpixel:
        assert_bits_equal(ctx.image(image), run.image(), f"{name}: replaced image")
    for o in range(octaves):
        for j in range(dogs + 1):
            assert_bits_equal(ctx.level("gaussian", o, j, image), run.level("gaussian", o, j), f"{name}: gaussian({o},{j}) img{image}")
            assert ctx.level_scale("gaussian", o, j) == run.scale("gaussian", o, j)
        for j in range(dogs):
            assert_bits_equal(ctx.level("dog", o, j, image), run.level("dog", o, j), f"{name}: dog({o},{j}) img{image}")
            assert ctx.level_scale("dog", o, j) == run.scale("dog", o, j)
    compare_gradient_maps(ctx, run, image, dogs, octaves, name, rep)
    for stage in ("candidates", "after_sort1", "after_orient", "after_sort2", "final"):
        got = ctx.stage(stage, image)
        want, wdesc = run.points(stage)
        rep[stage] = int(want.size)
        assert got.size == want.size, f"{name}: {stage}: {got.size} points vs oracle {want.size}"
        for f in ("x", "y", "octave", "index"):
            assert (got[f] == want[f]).all(), f"{name}: {stage}: field {f} differs at {int((got[f] != want[f]).sum())} points"
        assert (got["scale"] == want["scale"]).all(), f"{name}: {stage}: scale differs"
        if stage in ("candidates", "after_orient", "after_sort2", "final"):
            assert (got["filtered"].astype(bool) == want["filtered"].astype(bool)).all(), f"{name}: {stage}: filtered flags differ"
        if stage in ("after_orient", "after_sort2", "final"):
            m = ~want["filtered"].astype(bool)
            assert_bits_equal(got["orientation"][m], want["orientation"][m], f"{name}: {stage}: orientation")


def compare_run(ctx, img, dogs, octaves, subpixel, name, report_dir, batch_of=1, sigma=1.6, k=O.K_SQRT2, run=None):
    """`batch_of` copies of `img` in one batch against the oracle's run of it (`run`: that run, where the caller shares one among
    several tests - it is only read)."""
    params = _lib.Params(dogs, octaves, sigma, k, 1 if subpixel else 0)
    if run is None:
        run = O.OracleRun(img, dogs, octaves, sigma=sigma, k=k, subpixel=subpixel)
    assert run.status == 0, run.error
    imgs = np.stack([img] * batch_of)
    ctx.calculate_batch(imgs, params)
    rep = {"case": name}
    for image in sorted({0, batch_of - 1}):
        compare_image(ctx, run, image, dogs, octaves, subpixel, name, rep)
    counts = ctx.counts()
    kp, desc = ctx.results()
    want, wdesc = run.points("final")
    assert (counts == want.size).all()
    for image in range(batch_of):
        d = desc[image * want.size:(image + 1) * want.size]
        l2 = np.sqrt(((d.astype(np.float64) - wdesc) ** 2).sum(axis=1)) if want.size else np.zeros(0)
        rep["desc_max_l2"] = float(l2.max()) if l2.size else 0.0
        rep["desc_bit_exact"] = bool(d.tobytes() == wdesc.tobytes())
        assert (l2 <= DESC_TOL).all(), f"{name}: descriptors off by up to {l2.max()} (tol {DESC_TOL})"
        assert rep["desc_bit_exact"], f"{name}: descriptors within tolerance but not bit-exact ({int((d != wdesc).sum())} values)"
        recs = kp[image * want.size:(image + 1) * want.size]
        assert (recs["has_descriptor"] == (want["n_desc"] == 128)).all()
    with open(os.path.join(report_dir, "pipeline.jsonl"), "a") as f:
        f.write(json.dumps(rep) + "\n")
    return rep


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pipeline_parity(ctx, report_dir, case):
    name, w, h, seed, dogs, octaves, subpixel = case
    rep = compare_run(ctx, synth_frame(w, h, seed), dogs, octaves, subpixel, name, report_dir)
    assert rep["final"] > 0


def test_pipeline_parity_dense_keypoints(ctx, report_dir):
    """A lattice of blobs (sift_amd.synthetic.blob_frame): 0.06 keypoints per pixel, ~140 records in the 3x3 grid cells around
    a keypoint and windows covered tens of times over: the descriptor kernel's crowded-neighbourhood path (more records than a
    wave holds) and long per-pixel chains (sift.cpp:80-92), bit for bit."""
    from sift_amd.synthetic import blob_frame
    rep = compare_run(ctx, blob_frame(352, 264, 5), 3, 3, False, "blob lattice 352x264", report_dir)
    assert rep["final"] > 3000


STREAM_CASES = [
    ("streaming 320x250", 320, 250, 4, 3, 3, 1),
    ("streaming 322x250 (2 columns per lane only)", 322, 250, 12, 3, 3, 1),
    ("streaming 1024x768 4x3", 1024, 768, 13, 3, 4, 1),
    ("streaming 640x480 x3 frames", 640, 480, 14, 3, 3, 3),
    ("streaming 768x576 4 dogs x2 frames", 768, 576, 15, 4, 2, 2),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_pipeline_parity_streaming_blur(ctx, report_dir, case):
    """Whole pipeline with every blur of radius <= 14 (and the decimating blur of reduceToNextLevel) forced onto the
    streaming kernels, which otherwise only take launches of >= 1024 waves."""
    name, w, h, seed, dogs, octaves, batch_of = case
    ctx.set_option("stream_min_waves", 1)
    try:
        rep = compare_run(ctx, synth_frame(w, h, seed), dogs, octaves, False, name, report_dir, batch_of=batch_of)
        assert rep["final"] > 0
    finally:
        ctx.set_option("stream_min_waves", 0)


REDUCE_CASES = [
    # name, w, h, seed, octaves, frames
    ("kept-pixels reduce 640x480 (runs of 160: 4 columns per lane)", 640, 480, 31, 4, 2),
    ("kept-pixels reduce 1000x600 (runs of 250: 2 columns per lane)", 1000, 600, 32, 3, 1),
    ("kept-pixels reduce 641x479 (odd sizes: no parity split)", 641, 479, 33, 3, 2),
    ("kept-pixels reduce 1280x360 (several strips per run)", 1280, 360, 34, 3, 1),
    ("kept-pixels reduce 328x248 (run of 82 then 41/41: falls back where a run is odd)", 328, 248, 35, 3, 3),
]


@pytest.mark.parametrize("case", REDUCE_CASES, ids=[c[0] for c in REDUCE_CASES])
def test_pipeline_parity_kept_pixels_reduce(ctx, report_dir, case):
    """reduceToNextLevel as the blur that evaluates only the kept pixels (kernels_reduce.hip: de-interleaved LDS rows, column
    pass on kept rows), forced onto small inputs: every level of every octave (each next octave is seeded by it), stage lists
    and descriptors against the oracle.  (The odd sizes and the odd run fall back by themselves to the streaming blur that
    stores the kept quarter; that form forced on every shape is one of tests/diag_fallbacks.py's cases.)"""
    name, w, h, seed, octaves, frames = case
    ctx.set_option("stream_min_waves", 1)
    try:
        rep = compare_run(ctx, synth_frame(w, h, seed), 3, octaves, False, name, report_dir, batch_of=frames)
        assert rep["final"] > 0
    finally:
        ctx.set_option("stream_min_waves", 0)


PAIR_CASES = [
    # name, w, h, seed, dogs, octaves, subpixel, frames, sigma
    ("pair 640x480 (three strips, the last pulled left)", 640, 480, 1, 3, 4, False, 2, 1.6),
    ("pair 240x100 (one strip, both edges in it)", 240, 100, 2, 3, 2, False, 1, 1.6),
    ("pair 244x120 (second strip 4 columns in: a left halo partly outside)", 244, 120, 3, 3, 2, False, 2, 1.6),
    ("pair 484x200 (middle strip's right halo outside the image)", 484, 200, 4, 3, 2, False, 1, 1.6),
    ("pair 320x240 subpixel (the doubled image is the input)", 320, 240, 5, 3, 3, True, 1, 1.6),
    ("pair 1920x1080 config 3's frame", 1920, 1080, 6, 3, 4, False, 2, 1.6),
    ("pair 400x300 sigma 1.0 (radius 3)", 400, 300, 7, 3, 2, False, 1, 1.0),
    ("pair 400x300 sigma 1.3 (radius 4)", 400, 300, 8, 3, 2, False, 2, 1.3),
    ("pair 400x1000 sigma 2.0 (radius 6, tall: many chunks)", 400, 1000, 9, 4, 2, False, 1, 2.0),
]


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_pipeline_parity_first_two_levels_in_one_launch(ctx, report_dir, case):
    """Option blur_pair (default on; taken by batches that fill the chip): g(0,0) and g(0,1) from one launch (kernels_pair.hip: the
    second blur reads the first one's rows from LDS, reflected columns and rows included), forced onto small inputs and cut into
    many chunks: every level, stage list and the descriptors against the oracle."""
    name, w, h, seed, dogs, octaves, subpixel, frames, sigma = case
    ctx.set_option("blur_pair", 1)
    ctx.set_option("stream_min_waves", 1)
    ctx.set_option("pair_waves", 64 * frames)
    try:
        rep = compare_run(ctx, synth_frame(w, h, seed), dogs, octaves, subpixel, name, report_dir, batch_of=frames, sigma=sigma)
        assert rep["final"] > 0
        ctx.set_option("pair_waves", 0)
        compare_run(ctx, synth_frame(w, h, seed), dogs, octaves, subpixel, name + " [default cut]", report_dir, batch_of=frames, sigma=sigma)
    finally:
        ctx.set_option("stream_min_waves", 0)
        ctx.set_option("pair_waves", 0)


def test_release_library_rejects_measurement_options(ctx):
    """The shipped library knows eight options.  The names that force a fallback path exist only in libsift_hip_diag.so (this
    library's kernels with context.cpp compiled -DSIFT_HIP_DIAG: tests/diag_fallbacks.py), the ones that switch phases of kernels
    off for timing (wrong results) only in the ablation build (`make -C sift_amd/csrc ablate`); the shipped library answers
    SIFT_HIP_EINVAL for them, as it does for the variants removed in rounds 4 and 6 and for any unknown name."""
    for name in ("profile", "wire_count", "host_threads", "spin_wait", "orient_general", "stream_min_waves", "blur_pair", "pair_waves"):
        assert ctx._L.sift_hip_set_option(ctx._h, name.encode(), 0) == _lib.OK, name
    ctx.set_option("spin_wait", 1)
    ctx.set_option("blur_pair", 1)
    for name in ("fused_blur", "fused_edge", "fused_reduce", "reduce_kept", "dog_in_extrema", "gpu_cleanup", "pyramid_side", "gate_schedule",
                 "desc_dbg", "orient_dbg", "diag_repeat", "diag_pyramid_span", "diag_serial_gradient", "diag_cleanup_stamps", "stream_waves",
                 "chain_from", "chain_mode", "chain_spread", "gate_mid", "gate_early_chain", "extrema_stream", "io_kernels", "stage_kernels",
                 "fused_grid", "lazy_top", "tail_async", "tail_kernel", "desc_kernel", "no_such_option"):
        assert ctx._L.sift_hip_set_option(ctx._h, name.encode(), 1) == _lib.EINVAL, name


def test_forced_fallback_paths_in_the_diag_library():
    """tests/diag_fallbacks.py in a process of its own, against sift_amd/lib/libsift_hip_diag.so: the fallback paths the library
    takes by itself for shapes its default kernels do not fit, FORCED onto ordinary inputs and compared with the oracle - the
    two-pass blur, the unfused scan / edge filter with the pyramid writing its DoG levels, blur then resampling, the
    streaming decimating blur, std::sort on the host, the pyramid on one stream, the phase gate's other schedule."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SIFT_HIP_LIBRARY="libsift_hip_diag.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "diag_fallbacks.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" not in r.stdout, tail


def test_pipeline_parity_general_orientation_bins(ctx, report_dir):
    """The orientation histogram's per-sample-bin form (never selected by real frames: App. B-9 puts every sample
    in bin 0, which the gradient pass detects) gives the same results as the all-zero-bins fast path."""
    ctx.set_option("orient_general", 1)
    try:
        compare_run(ctx, synth_frame(640, 480, 21), 3, 3, False, "general orientation bins 640x480", report_dir, batch_of=2)
    finally:
        ctx.set_option("orient_general", 0)


def test_pipeline_parity_bench_workload(ctx, report_dir):
    """The bench's own launch shapes: 32 frames of 1920x1080, 3 DoGs x 4 octaves (BASELINE.json configs[4]); every
    level, stage and descriptor of the first and last frame against the oracle."""
    rep = compare_run(ctx, synth_frame(1920, 1080, 3), 3, 4, False, "bench workload 32 x 1080p", report_dir, batch_of=32)
    assert rep["final"] > 0


def test_pipeline_parity_bench_frames(ctx, report_dir):
    """The bench's own CONTENT: synth_frame(1920, 1080, s) for s = 1..32 (what bench.py's rank 0 runs), 32 distinct frames in
    ONE batch, so every image of the launch has its own candidate count, cleanup rounds, list offsets and output offset
    (sift.cpp:37-54 per image).  Every frame: every stage list (coordinates, octave / index, scale, flags, orientations),
    the per-image counts, the keypoint records and all descriptors, bit for bit against the oracle; three frames also every
    Gaussian and DoG level; frame 1 also against what the reference's own binary returned for it."""
    import hashlib
    dogs, octaves = 3, 4
    frames = np.stack([synth_frame(1920, 1080, s) for s in range(1, 33)])
    ctx.calculate_batch(frames, _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, 0))
    counts = ctx.counts().copy()
    kp, desc = ctx.results()
    kp, desc = kp.copy(), desc.copy()
    assert len(set(counts.tolist())) > 16, "the frames should differ in their keypoint counts"
    base, rep = 0, {"case": "bench frames 1..32 in one batch", "counts": counts.tolist()}
    for i in range(32):
        run = O.OracleRun(frames[i], dogs, octaves)
        assert run.status == 0, run.error
        for stage in ("candidates", "after_sort1", "after_orient", "after_sort2", "final"):
            got = ctx.stage(stage, i)
            want, wdesc = run.points(stage)
            assert got.size == want.size, f"frame {i + 1}: {stage}: {got.size} points vs oracle {want.size}"
            for f in ("x", "y", "octave", "index"):
                assert (got[f] == want[f]).all(), f"frame {i + 1}: {stage}: field {f}"
            assert got["scale"].tobytes() == want["scale"].tobytes(), f"frame {i + 1}: {stage}: scale"
            if stage != "after_sort1":
                assert (got["filtered"].astype(bool) == want["filtered"].astype(bool)).all(), f"frame {i + 1}: {stage}: filtered"
            if stage in ("after_orient", "after_sort2", "final"):
                m = ~want["filtered"].astype(bool)
                assert_bits_equal(got["orientation"][m], want["orientation"][m], f"frame {i + 1}: {stage}: orientation")
        want, wdesc = run.points("final")
        assert counts[i] == want.size, f"frame {i + 1}: count"
        k = kp[base:base + want.size]
        for f in ("x", "y", "octave", "index"):
            assert (k[f] == want[f]).all(), f"frame {i + 1}: result field {f}"
        assert k["scale"].tobytes() == want["scale"].tobytes() and k["orientation"].tobytes() == want["orientation"].tobytes()
        assert (k["has_descriptor"] == (want["n_desc"] == 128)).all()
        assert desc[base:base + want.size].tobytes() == wdesc.tobytes(), f"frame {i + 1}: descriptors"
        if i in (0, 13, 31):
            for o in range(octaves):
                for j in range(dogs + 1):
                    assert_bits_equal(ctx.level("gaussian", o, j, i), run.level("gaussian", o, j), f"frame {i + 1}: gaussian({o},{j})")
                for j in range(dogs):
                    assert_bits_equal(ctx.level("dog", o, j, i), run.level("dog", o, j), f"frame {i + 1}: dog({o},{j})")
        if i == 0:
            pin_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_bench_frame.npz")
            if os.path.exists(pin_path):     # the reference binary's own answer for frame 1
                pin = np.load(pin_path)
                ref = pin["points"]
                assert k.size == ref.size
                for f in ("x", "y", "octave", "index"):
                    assert (k[f] == ref[f]).all(), f
                assert k["scale"].tobytes() == ref["scale"].tobytes() and k["orientation"].tobytes() == ref["orientation"].tobytes()
                d0 = desc[base:base + want.size]
                assert hashlib.sha256(d0[k["has_descriptor"].astype(bool)].tobytes()).hexdigest() == str(pin["desc_sha"])
                rep["frame1_equals_reference_binary"] = True
        run.close()
        base += want.size
    assert base == kp.size
    with open(os.path.join(report_dir, "pipeline.jsonl"), "a") as f:
        f.write(json.dumps(rep) + "\n")


def test_bench_starts_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` as a BARE command (no torch.distributed.run, no WORLD_SIZE): the parent starts two fresh
    rank processes before touching the GPU and passes rank 0's one JSON line through.  Both ranks share this box's one GPU, so the
    transport is gloo; the flow (block-sharded seeds, per-step gather of the keypoint lists on rank 0, barrier + max-over-ranks
    timing) is the N > 1 flow."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-device", "--backend", "gloo",
                        "--steps", "2", "--warmup", "1", "--frames", "4", "--no-cpu-baseline", "--no-extras"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout   # ONE line on stdout: RCCL's banner and the other ranks' output go to stderr
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["frames_total"] == 8
    assert out["config"]["gather_steps_on_rank0"] == 2
    assert out["config"]["gather_keypoints_on_rank0"] == out["config"]["keypoints_per_step"] * 2
    assert out["config"]["rccl_ranks"] == 0      # gloo: no RCCL communicator in this run, and the line says so
    assert out["value"] > 0 and out["roofline"]["frac"] > 0
    # a failing rank makes the command fail (here: a library option that does not exist)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-device", "--backend", "gloo",
                        "--steps", "1", "--warmup", "0", "--frames", "2", "--no-cpu-baseline", "--no-extras", "--set", "no_such_option=1"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0


def test_bench_rccl_loopback_prints_one_line():
    """`bench.py --rccl-loopback`: the N > 1 per-rank step on one GPU, the keypoint lists looped through RCCL.  RCCL prints its
    version banner to stdout when the communicator is created; the bench's contract is ONE JSON line there, so the line goes to a
    private copy of stdout and everything else to stderr."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--rccl-loopback", "--steps", "3", "--warmup", "1", "--frames", "4",
                        "--no-cpu-baseline", "--no-extras"], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["config"]["gather_steps_on_rank0"] >= 3 and out["value"] > 0


def test_bench_plain_run_dumps_the_last_steps_outputs(ctx, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` does the timed steps only (the legs with runs of their own wait behind
    `--full`), and `--dump-outputs DIR` writes what the last timed step returned as float arrays: here they must be what a
    context of this process returns for the same frames (seeds 1 and 2), row for row, bit for bit."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    dump = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "2",
                        "--dump-outputs", dump], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "keypoints/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0 and abs(out["value"] - out["config"]["keypoints_per_step"] / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["ms_per_step_repeats"]["n"] == 1
    for key in ("cpu_baseline", "parity_spot_check", "host_inclusive", "single_frame_ms", "dropin_cpp"):
        assert key not in out, key
    assert "frac_alone" not in out["roofline"] and out["roofline"]["traffic"] is None and out["roofline"]["frac"] > 0

    got = {n: np.load(os.path.join(dump, n + ".npy")) for n in ("counts", "sample_rows", "keypoints", "descriptors")}
    assert sorted(os.listdir(dump)) == sorted(n + ".npy" for n in got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(os.path.join(dump, f)) for f in os.listdir(dump)) <= 64 * 1000 * 1000
    frames = np.stack([synth_frame(1920, 1080, s) for s in (1, 2)])
    ctx.calculate_batch(frames, _lib.Params(3, 4, 1.6, O.K_SQRT2, 0))
    kp, desc = ctx.results()
    assert np.array_equal(got["counts"], ctx.counts().astype(np.float64))
    assert kp.size == out["config"]["keypoints_per_step"] and kp.size > 0
    rows = got["sample_rows"].astype(np.int64)
    assert np.array_equal(rows, np.arange(kp.size))      # fewer keypoints than the sample holds: every row is there
    for col, f in enumerate(("x", "y", "octave", "index", "scale", "orientation", "filtered", "has_descriptor")):
        assert got["keypoints"][:, col].astype(kp.dtype[f]).tobytes() == np.ascontiguousarray(kp[f][rows]).tobytes(), f
    assert got["descriptors"].dtype == np.float32 and got["descriptors"].tobytes() == np.ascontiguousarray(desc[rows]).tobytes()


@pytest.mark.parametrize("host_loop", ["stream", "dispatch"])
def test_bench_eight_ranks_sharing_the_gpu(host_loop):
    """BASELINE config 4's world size on this one-GPU box: `bench.py --gpus 8` with all eight ranks on GPU 0 (gloo as the
    transport), 4 frames per rank = seeds 1 .. 32 block-sharded.  `--check-gather` makes rank 0 run all 32 frames itself after
    the timed region and compare the lists that came through the gather in the last step with its own: records, descriptor
    floats and per-image counts, in global image order.  Both host loops: every context's thread feeding itself with one
    gather thread per rank (the default), and the single dispatching thread."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--share-device", "--backend", "gloo",
                        "--steps", "3", "--warmup", "1", "--frames", "4", "--no-cpu-baseline", "--no-extras", "--check-gather",
                        "--host-loop", host_loop],
                       env=env, cwd=root, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout   # ONE line on stdout: RCCL's banner and the other ranks' output go to stderr
    out = json.loads(lines[0])
    cfg = out["config"]
    assert out["n_gpus"] == 8 and out["steps"] == 3 and cfg["frames_total"] == 32 and cfg["host_loop"] == host_loop
    assert cfg["gather_steps_on_rank0"] == 3
    assert cfg["gather_keypoints_on_rank0"] == cfg["keypoints_per_step"] * 3
    assert cfg["gather_check"] is True, cfg.get("gather_check_what")
    assert out["value"] > 0


def test_pipeline_parity_256_frame_batch(ctx, report_dir):
    """BASELINE.json configs[3]'s whole 256-frame batch on one GPU: every level buffer is larger than 2^31 bytes, so
    any 32-bit byte offset would show in the last frame."""
    rep = compare_run(ctx, synth_frame(1920, 1080, 5), 3, 4, False, "256 x 1080p on one GPU", report_dir, batch_of=256)
    assert rep["final"] > 0


def test_batch_images_independent(ctx, report_dir):
    """Every frame of a batch gets the single-frame result (frames differ)."""
    params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    frames = np.stack([synth_frame(256, 192, s) for s in (1, 2, 3)])
    ctx.calculate_batch(frames, params)
    counts = ctx.counts()
    kp, desc = ctx.results()
    base = 0
    for i in range(3):
        want, wdesc = O.OracleRun(frames[i], 3, 3).points("final")
        assert counts[i] == want.size
        k = kp[base:base + counts[i]]
        assert (k["x"] == want["x"]).all() and (k["y"] == want["y"]).all() and (k["octave"] == want["octave"]).all()
        assert desc[base:base + counts[i]].tobytes() == wdesc.tobytes()
        base += counts[i]


def check_u8_frames_in_sparse_lists_out(ctx, frames, params, min_keypoints):
    """8-bit frames in, sparse lists out, for the 8-bit valued float frames `frames` under `params`: bit for bit the float path's
    keypoints and descriptors, from pageable and from page-locked memory; level 1 of every octave of the last frame against the
    oracle.  -> (counts, keypoint records, descriptors) of the float path."""
    from sift_amd.sift import pinned_array, unpack_sparse_host
    dogs, octaves = params.dogs_per_epoch, params.octaves
    u8 = frames.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), frames)                            # the generator's frames are 8-bit valued
    ctx.calculate_batch(frames, params)
    wcounts, (wkp, wdesc) = ctx.counts().copy(), tuple(a.copy() for a in ctx.results())
    assert wkp.size > min_keypoints
    pin = pinned_array(u8.shape, np.uint8)
    pin[...] = u8
    last = len(frames) - 1
    run = O.OracleRun(frames[last], dogs, octaves, sigma=params.sigma, k=params.k, subpixel=bool(params.subpixel))
    for src in (u8, pin):
        ctx.calculate_batch(src, params)
        assert ctx.counts().tolist() == wcounts.tolist()
        kp, desc = ctx.results()
        assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
        for o in range(octaves):
            assert_bits_equal(ctx.level("gaussian", o, 1, last), run.level("gaussian", o, 1), f"g({o},1)")
        rec, val = ctx.results_sparse()
        assert rec.shape == (wkp.size, 34) and val.size == int((wdesc.view(np.uint32) != 0).sum())
        for threads in (1, 5):
            kp2, desc2 = unpack_sparse_host(rec, val, threads=threads)
            assert kp2.tobytes() == wkp.tobytes() and desc2.tobytes() == wdesc.tobytes()
        prec, pval = pinned_array((wkp.size + 7, 34), np.uint8), pinned_array((val.size + 100,), np.float32)
        rec3, val3 = ctx.results_sparse(prec, pval)
        assert rec3.tobytes() == rec.tobytes() and val3.tobytes() == val.tobytes()
    return wcounts, wkp, wdesc


def test_u8_frames_in_sparse_lists_out(ctx):
    """The boundary for a host that holds 8-bit frames (the reference's inputs are 8-bit files, main.cpp:52-54): uint8 in
    (sift_hip_calculate_batch_u8: widened on the GPU to the floats vigra::importImage yields), sparse lists out
    (sift_hip_result_copy_sparse + sift_hip_sparse_unpack_host) - bit for bit the float path's keypoints and descriptors, from
    pageable and from page-locked memory, and for a batch without a keypoint."""
    from sift_amd.sift import unpack_sparse_host
    params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    frames = np.stack([synth_frame(333, 257, 70 + i) for i in range(5)])          # odd sizes: the scalar tail of the widening kernel
    check_u8_frames_in_sparse_lists_out(ctx, frames, params, 500)
    ctx.calculate_batch(np.full((2, 96, 128), 9, np.uint8), params)
    assert ctx.total() == 0
    rec, val = ctx.results_sparse()
    assert rec.shape == (0, 34) and val.size == 0 and unpack_sparse_host(rec, val)[0].size == 0


def test_constant_image_has_no_keypoints(ctx):
    """Every interior pixel ties => candidate; H = 0 => inverse fails => all filtered."""
    img = np.full((96, 128), 77.0, np.float32)
    params = _lib.Params(3, 2, 1.6, O.K_SQRT2, 0)
    ctx.calculate_batch(img[None], params)
    cand = ctx.stage("candidates")
    run = O.OracleRun(img, 3, 2)
    assert cand.size == run.points("candidates")[0].size == (128 - 2) * (96 - 2) + (64 - 2) * (48 - 2)
    assert cand["filtered"].all()
    assert ctx.counts()[0] == 0


def test_exception_parity(ctx):
    """B-13: pyramid level not larger than the kernel radius; asserts; B-14 dead 16x16 blur."""
    img = synth_frame(160, 120, 1)
    for (dogs, octaves) in [(3, 4), (5, 3)]:
        run = O.OracleRun(img, dogs, octaves)
        assert run.status == 1
        with pytest.raises(PreconditionViolation) as e:
            Sift(dogs, octaves, context=ctx).calculate(img)
        assert str(e.value) == run.error
    with pytest.raises(AssertionError):
        Sift(2, 3, context=ctx).calculate(img)
    with pytest.raises(AssertionError):
        Sift(3, 0, context=ctx).calculate(img)
    # B-14: 4 DoGs per octave, 3 octaves: DoG (2,2) has scale 3.2*... => dead blur radius > 15
    big = synth_frame(512, 384, 3)
    run = O.OracleRun(big, 4, 3)
    if run.status == 1:
        with pytest.raises(PreconditionViolation) as e:
            Sift(4, 3, context=ctx).calculate(big)
        assert str(e.value) == run.error
    else:
        compare_run(ctx, big, 4, 3, False, "512x384 4 dogs 3 oct", os.path.join(os.path.dirname(__file__), "..", "gpurun_out", "parity"))


def test_full_size_properties(ctx):
    """1920x1080, 4 oct x 3 DoG (bench workload): size-independent properties + oracle counts."""
    img = synth_frame(1920, 1080, 1)
    params = _lib.Params(3, 4, 1.6, O.K_SQRT2, 0)
    ctx.calculate_batch(img[None], params)
    kp, desc = ctx.results()
    assert kp.size > 1000
    # orientation is the rank-deficient parabola vertex ~177.4913 for every keypoint (B-9)
    assert np.all(np.abs(kp["orientation"] - 177.4913) < 1e-3)
    d = desc.reshape(-1, 16, 8)
    assert np.all(d[:, :, 7] == 0)                      # bin 7 is never written (% 7)
    s = d.sum(axis=2)
    assert np.all((np.abs(s - 1) < 1e-5) | (s == 0))    # each cell L1-normalised
    assert np.all(kp["x"] >= 8) and np.all(kp["y"] >= 8)
    run = O.OracleRun(img, 3, 4)
    want, wdesc = run.points("final")
    assert kp.size == want.size
    assert (kp["x"] == want["x"]).all() and (kp["y"] == want["y"]).all() and (kp["octave"] == want["octave"]).all()
    assert desc.tobytes() == wdesc.tobytes()


# ------------------------------------------------------------------------------------------------
# committed golden fixtures (tests/golden/, made by make_golden.py in the dev container)
# ------------------------------------------------------------------------------------------------
from golden_util import CASES as GOLDEN_CASES, load_case, sha  # noqa: E402


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_hip_matches_golden(ctx, name):
    g, img, dogs, octaves, subpixel = load_case(name)
    ctx.calculate_batch(img[None], _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, 1 if subpixel else 0))
    for k, want in zip(g["level_names"], g["level_sha"]):
        kind = "gaussian" if k[0] == "g" else "dog"
        o, j = map(int, k[1:].split("_"))
        assert sha(ctx.level(kind, o, j)) == want, k
    got = [ctx.stage(s).size for s in ("candidates", "after_sort1", "after_orient", "after_sort2", "final")]
    assert got == g["counts"].tolist()
    cand = ctx.stage("candidates")
    assert sha(cand["filtered"].astype(np.uint8)) == str(g["cand_flags_sha"])
    kp, desc = ctx.results()
    assert (kp["x"] == g["kp_x"]).all() and (kp["y"] == g["kp_y"]).all() and (kp["octave"] == g["kp_octave"]).all()
    assert kp["orientation"].tobytes() == g["kp_orientation"].tobytes()
    assert desc.tobytes() == g["descriptors"].tobytes()


def test_config5_4k_subpixel_digest(ctx):
    """BASELINE config 5: 3840x2160, subpixel, 3 DoGs.  6 octaves makes the reference throw in the dead 16x16
    blur of an octave-5 keypoint (App. B-14): same message here; 5 octaves runs: counts of every stage and
    SHA-256 of keypoints, orientations, scales and descriptors equal the oracle's (tests/golden/digest_*.npz,
    make_golden.py config5 — the oracle needs minutes for this frame).  Also covers the paths only big
    frames take: > 2^20 candidates per image (global-memory sort keys) and > 4096 descriptor tiles."""
    from golden_util import GOLDEN
    g = np.load(os.path.join(GOLDEN, "digest_config5_4k.npz"))
    dogs, octaves, subpixel, w, h, seed = (int(v) for v in g["meta"])
    img = synth_frame(w, h, seed)
    with pytest.raises(PreconditionViolation) as e:
        ctx.calculate_batch(img[None], _lib.Params(dogs, int(g["throw_octaves"]), 1.6, O.K_SQRT2, subpixel))
    assert str(e.value) == str(g["throw_message"])
    ctx.calculate_batch(img[None], _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, subpixel))
    got = [ctx.stage(s).size for s in ("candidates", "after_sort1", "after_orient", "after_sort2", "final")]
    assert got == g["counts"].tolist()
    kp, desc = ctx.results()
    assert sha(np.stack([kp["x"], kp["y"], kp["octave"], kp["index"]], 1).astype(np.uint16)) == str(g["kp_sha"])
    assert sha(kp["orientation"]) == str(g["orientation_sha"])
    assert sha(kp["scale"]) == str(g["scale_sha"])
    assert sha(desc) == str(g["descriptors_sha"])


def test_u16_size_truncation_in_the_pipeline(ctx):
    """App. B-7 end to end: on this 3840x2160 frame 80523 points survive the edge filter, the reference's
    `u16_t size` (sift.cpp:41) keeps 80523 mod 65536 = 14987 of them, and everything downstream (orientation
    stage run late in list order, second cleanup, descriptors) follows from that list."""
    from golden_util import GOLDEN
    g = np.load(os.path.join(GOLDEN, "digest_u16_truncation_4k.npz"))
    dogs, octaves, subpixel, w, h, seed = (int(v) for v in g["meta"])
    ctx.calculate_batch(synth_frame(w, h, seed)[None], _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, subpixel))
    got = [ctx.stage(s).size for s in ("candidates", "after_sort1", "after_orient", "after_sort2", "final")]
    assert got == g["counts"].tolist()
    assert got[1] == 14987
    kp, desc = ctx.results()
    assert sha(np.stack([kp["x"], kp["y"], kp["octave"], kp["index"]], 1).astype(np.uint16)) == str(g["kp_sha"])
    assert sha(kp["orientation"]) == str(g["orientation_sha"])
    assert sha(desc) == str(g["descriptors_sha"])


# ------------------------------------------------------------------------------------------------
# cleanup (std::sort + u16 truncation) as a GPU kernel vs libstdc++ itself
# ------------------------------------------------------------------------------------------------
def _survivors(ctx, flags, on_gpu):
    import ctypes as C
    flags = np.ascontiguousarray(flags, np.uint8)
    out = np.zeros(max(flags.size, 1), np.int32)
    cnt = C.c_int32()
    rc = ctx._L.sift_hip_cleanup_survivors(ctx._h, flags, flags.size, out, C.byref(cnt), on_gpu)
    assert rc == 0
    return out[:cnt.value].copy()


def test_cleanup_kernel_matches_std_sort(ctx):
    rng = np.random.default_rng(7)
    cases = []
    for n in list(range(0, 40)) + [63, 64, 65, 100, 257, 1000, 1023, 1024, 1025, 2049, 5000, 20000, 70000, 200000]:
        for p in (0.0, 0.03, 0.2, 0.5, 0.8, 0.9, 0.97, 1.0):
            cases.append((rng.random(n) < p).astype(np.uint8))
    for n in (100, 1000, 4097, 66000):   # structured inputs
        a = np.zeros(n, np.uint8); a[n // 2:] = 1; cases.append(a)
        cases.append(a[::-1].copy())
        b = np.zeros(n, np.uint8); b[::2] = 1; cases.append(b)
        c = np.ones(n, np.uint8); c[::17] = 0; cases.append(c)
    for flags in cases:
        perm = O.sort_by_filter(flags)
        nz = int((flags == 0).sum())
        want = perm[:nz & 0xffff]                       # u16_t size (sift.cpp:41)
        host = _survivors(ctx, flags, 0)
        assert host.size == want.size and (host == want).all(), (flags.size, "host glue")
        for variant in (1, 2):   # keys in LDS bits / keys in global bytes
            gpu = _survivors(ctx, flags, variant)
            assert gpu.size == want.size and (gpu == want).all(), (flags.size, float(flags.mean()) if flags.size else 0, "gpu kernel", variant)


def expected_result_file(tmp_path, img, dogs, octaves, subpixel=False):
    """interstpoints.txt as the reference's main.cpp:78-89 writes it for the oracle's points (C++ iostream formatting)."""
    run = O.OracleRun(img, dogs, octaves, subpixel=subpixel)
    path = tmp_path / "expected_interstpoints.txt"
    run.write_result(path)
    return open(path, "rb").read(), run


def check_overlay(png_path, src_bgr, run, subpixel):
    """<img>_orientation.png = the colour image with the boxes of main.cpp:60-73 for the oracle's points, drawn by the
    independent restatement of cv::RotatedRect::points / cv::line in tests/overlay_ref.py."""
    from sift_amd import cli
    pts, desc = run.points("final")
    kp = np.zeros(pts.size, _lib.KEYPOINT_DTYPE)
    for f in ("scale", "orientation", "x", "y", "octave", "index"):
        kp[f] = pts[f]
    import overlay_ref
    want = overlay_ref.draw_overlay(src_bgr, kp, bool(subpixel))   # the independent renderer, not the library's own
    got = cli.read_image_bgr(str(png_path))
    assert np.array_equal(got, want)
    assert (got != src_bgr).any()


RUNTIME_CRASH_ATTEMPTS = 1


def _run_past_runtime_crashes(cmd, **kw):
    """Run a multi-threaded C++ host of the library - ONCE.  Rounds 2 - 4 repeated a run that died of SIGSEGV / SIGABRT up to eight
    times: HIP 7.2's hipLaunchKernel looks the kernel's host stub up on every launch, and that lookup returned null in 0 - 23 % of
    the runs of such hosts (profiles/r04_soak.txt).  Since round 5 the library resolves every kernel's function object once per
    device and launches through hipExtModuleLaunchKernel (sift_amd/csrc/launch_cache.h): 0 crashes in 300 runs against 13 in 300
    for the runtime's own path, alternately on one box (profiles/r05_launch_ab_soak.txt) - so a crash is a failure again."""
    import subprocess
    out = None
    for attempt in range(RUNTIME_CRASH_ATTEMPTS):
        out = subprocess.run(cmd, capture_output=True, text=True, **kw)
        if out.returncode not in (-11, -6):
            break
    return out


def test_cpp_dropin_example(ctx, tmp_path):
    """examples/sift_points.cpp (the C++ sift::Sift drop-in over the C ABI, shaped like the reference's main.cpp) on the parrot
    fixture: interstpoints.txt equals, byte for byte, what main.cpp:78-89 writes for the oracle's points; the overlay PNG
    holds main.cpp:60-73's boxes; a PNG input is read without PIL; exceptions reach the caller with Vigra's text."""
    import shutil
    import subprocess
    from sift_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sift_points"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_points.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    shutil.copy(os.path.join(root, "tests", "golden", "parrot_r.pgm"), tmp_path / "parrot_r.pgm")
    out = subprocess.run([str(exe), "parrot_r.pgm", "4", "3", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    img = read_pgm(os.path.join(root, "tests", "golden", "parrot_r.pgm"))
    want, run = expected_result_file(tmp_path, img, 3, 4)
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want
    check_overlay(tmp_path / "parrot_r.pgm_orientation.png", cli.read_image_bgr(str(tmp_path / "parrot_r.pgm")), run, False)
    # an RGB PNG: band 0 (red) is what the pipeline sees, the overlay keeps the colours
    rgb = np.stack([synth_frame(200, 150, 7), synth_frame(200, 150, 8), synth_frame(200, 150, 9)], axis=2).astype(np.uint8)
    cli._err_call(_lib.load().sift_hip_png_write_bgr8, str(tmp_path / "rgb.png").encode(), np.ascontiguousarray(rgb[:, :, ::-1]).reshape(-1), 200, 150)
    out = subprocess.run([str(exe), "rgb.png", "3", "3", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want, run = expected_result_file(tmp_path, synth_frame(200, 150, 7), 3, 3, subpixel=True)
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want
    check_overlay(tmp_path / "rgb.png_orientation.png", np.ascontiguousarray(rgb[:, :, ::-1]), run, True)
    # exception text reaches the caller like vigra's would: 160x120 cannot carry 4 octaves
    small = synth_frame(160, 120, 1).astype(np.uint8)
    with open(tmp_path / "small.pgm", "wb") as f:
        f.write(b"P5\n160 120\n255\n" + small.tobytes())
    out = subprocess.run([str(exe), "small.pgm", "4", "3", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert "kernel longer than line" in out.stderr


def test_cpp_dropin_example_large_result(ctx, tmp_path):
    """examples/sift_points.cpp on a 1920x1080 frame (frame 1 of the bench batch, as an 8-bit PGM): 19 764 keypoints, so
    sift::Sift::collect (include/sift/sift.hpp) takes its parallel path - the sparse lists expanded by the object's worker threads,
    each into its own range of InterestPoints - and interstpoints.txt still equals, byte for byte, what main.cpp:78-89 writes for
    the oracle's points."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sift_points"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_points.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    img = synth_frame(1920, 1080, 1)
    assert (img == np.round(img)).all() and img.min() >= 0 and img.max() <= 255
    with open(tmp_path / "frame.pgm", "wb") as f:
        f.write(b"P5\n1920 1080\n255\n" + img.astype(np.uint8).tobytes())
    out = subprocess.run([str(exe), "frame.pgm", "4", "3", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    want, run = expected_result_file(tmp_path, img, 3, 4)
    assert run.points("final")[0].size > 4096          # the parallel path of collect()
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want


def test_cpp_gated_pair_example(ctx, tmp_path):
    """examples/sift_pipeline.cpp: two sift::Sift objects on two threads joined by a gate (sift_hip_gate_*, Sift::join)
    give, frame for frame, the single object's results."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sift_pipeline"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_pipeline.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-o", str(exe)])
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    out = _run_past_runtime_crashes([str(exe), os.path.join(root, "tests", "golden", "parrot_r.pgm"), "9"], cwd=tmp_path, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok: 9 frames"), out.stdout + out.stderr


def _run_isolated(script, timeout=900):
    """A test body that drives several host threads against the HIP runtime runs in a process of its own (a crash there must not
    take the whole test session with it).  One attempt: a run that dies, fails an assertion or ends in any other way fails the
    test (_run_past_runtime_crashes)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = ("import sys, numpy as np\n"
            f"sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + '/tests')\n"
            "import pytest, oracle_lib as O\n"
            "from sift_amd import _lib\n"
            "from sift_amd.sift import Group, Context, PreconditionViolation\n"
            "from sift_amd.synthetic import synth_frame\n")
    r = _run_past_runtime_crashes([sys.executable, "-c", head + script], timeout=timeout)
    assert r.returncode == 0 and "isolated ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


_GROUP_SHARDS_SCRIPT = """
params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
frames = np.stack([synth_frame(320, 240, 40 + i) for i in range(7)])       # 7 frames over 3 shards: 3 + 3 + 1
ctx = Context(0)
g = Group([0, 0, 0])
g.calculate_batch(frames, params)
ctx.calculate_batch(frames, params)
assert g.counts().tolist() == ctx.counts().tolist() and g.total() == ctx.total()
kp, desc = g.results()
wkp, wdesc = ctx.results()
assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
assert (g.status() == 0).all()
cms, gms, nbytes = g.timing()
assert cms > 0 and gms >= 0 and nbytes == 0                        # same device: nothing crossed a link
assert g.gather_exposed_ms() >= 0
g.calculate_batch(frames[:2], params)                              # fewer frames than shards
ctx.calculate_batch(frames[:2], params)
assert g.results()[1].tobytes() == ctx.results()[1].tobytes()
# what shards on other GPUs do (forced here for the shards of this one GPU): every shard packs its lists into the sparse
# wire format on its own device, the packed lists are collected and unpacked on the first device
for copy_kernels in (1, 0):                                        # the library's copy kernels / the runtime's copies
    g.set_option("copy_kernels", copy_kernels)
    g.set_option("gather_wire", 2)
    mixed = np.concatenate([frames, np.full((1, 240, 320), 3.0, np.float32)])   # the last shard's last frame has no keypoint
    g.calculate_batch(mixed, params)
    ctx.calculate_batch(mixed, params)
    assert g.counts().tolist() == ctx.counts().tolist() and g.total() == ctx.total()
    kp, desc = g.results()
    wkp, wdesc = ctx.results()
    assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
    g.set_option("gather_wire", 1)
    g.calculate_batch(mixed, params)
    assert g.results()[1].tobytes() == wdesc.tobytes()
with pytest.raises(PreconditionViolation) as e:                    # 160x120 cannot carry 4 octaves
    g.calculate_batch(np.stack([synth_frame(160, 120, 1)] * 4), _lib.Params(3, 4, 1.6, O.K_SQRT2, 0))
assert "kernel longer than line" in str(e.value)
g.close(); ctx.close()
print("isolated ok")
"""


def test_group_of_shards_matches_single_context(ctx):
    """sift_hip_group (SURVEY.md 8(e) as native host code): a batch block-sharded over three shards — all on this box's one
    GPU, which exercises the threads, the sharding, the per-image bookkeeping and the device-to-device gather — returns the
    single context's keypoints, descriptors, counts and status in global image order; a frame that "throws" (App. B-14) is
    reported like sift_hip_calculate_batch reports it.  (In a process of its own: see _run_isolated.)"""
    _run_isolated(_GROUP_SHARDS_SCRIPT)


_GROUP_PIPELINE_SCRIPT = """
params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
batches = [np.stack([synth_frame(320, 240, 300 + 8 * b + i) for i in range(5 + b % 3)]) for b in range(5)]
batches[3] = np.concatenate([batches[3], np.full((1, 240, 320), 5.0, np.float32)])     # a frame without keypoints
ctx = Context(0)
for wire in (1, 2):
    g = Group([0, 0, 0])
    g.set_option("gather_wire", wire)
    got = []
    g.submit(batches[0], params)
    for b in range(1, len(batches) + 1):
        if b < len(batches):
            g.submit(batches[b], params)
            if b == 1:
                with pytest.raises(ValueError):
                    g.submit(batches[0], params)
        g.collect()
        got.append((g.counts().copy(),) + tuple(a.copy() for a in g.results()))
    assert g.transport()[0] == 0                       # one GPU listed three times: RCCL takes one rank per GPU
    for b, (counts, kp, desc) in zip(batches, got):
        ctx.calculate_batch(b, params)
        wkp, wdesc = ctx.results()
        assert counts.tolist() == ctx.counts().tolist()
        assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
    g.close()
# batches that GROW while two are in flight: the pack buffers, arrival areas and result arrays of both slots and the shards'
# context buffers are reallocated under way - with deferred frees (launch_guard.h: no hipFree on a GPU while one of its
# transfers may be waiting for its peer; the retired allocations go when the group is idle)
from sift_amd.sift import lock_wait_ms
grow = [np.stack([synth_frame(320, 240, 700 + 16 * b + i) for i in range(3 * 2 ** b)]) for b in range(4)]      # 3, 6, 12, 24 frames
g = Group([0, 0, 0])
got = []
g.submit(grow[0], params)
for b in range(1, len(grow) + 1):
    if b < len(grow):
        g.submit(grow[b], params)
    g.collect()
    got.append((g.counts().copy(),) + tuple(a.copy() for a in g.results()))
for b, (counts, kp, desc) in zip(grow, got):
    ctx.calculate_batch(b, params)
    wkp, wdesc = ctx.results()
    assert counts.tolist() == ctx.counts().tolist()
    assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
g.close()
assert lock_wait_ms() >= 0.0
ctx.close()
print("isolated ok")
"""


def test_group_two_batches_in_flight(ctx):
    """sift_hip_group_submit / _collect: two batches in flight over three shards, the gather of batch k under the kernels of
    batch k+1 (pack buffers, arrival areas and result arrays double-buffered); every batch returns the single context's lists;
    a third submit without a collect is refused.  (In a process of its own: see _run_isolated.)"""
    _run_isolated(_GROUP_PIPELINE_SCRIPT)


_GROUP_RCCL_SCRIPT = """
import os, sys, numpy as np
os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")      # no network on the test boxes: RCCL's bootstrap stays on the loopback interface
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + '/tests')
from sift_amd import _lib
from sift_amd.sift import Group, Context, K_SQRT2
from sift_amd.synthetic import synth_frame
params = _lib.Params(3, 3, 1.6, K_SQRT2, 0)
g = Group([0])
g.set_option('gather_loopback', 1)
g.set_option('gather_transport', 2)      # RCCL or fail
used, why = g.transport()
assert used == 1, why
c = Context(0)
batches = [np.stack([synth_frame(320, 240, 500 + 4 * b + i) for i in range(3)]) for b in range(3)]
batches.append(np.full((2, 240, 320), 9.0, np.float32))        # a batch without a single keypoint
for wire in (1, 0):
    g.set_option('gather_wire', wire)
    for b in batches:
        g.calculate_batch(b, params)
        c.calculate_batch(b, params)
        kp, desc = g.results(); wkp, wdesc = c.results()
        assert g.counts().tolist() == c.counts().tolist()
        assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
        cms, gms, nbytes = g.timing()
        assert nbytes == (34 if wire else 532) * kp.size + (4 * int((desc.view(np.uint32) != 0).sum()) if wire else 0), (nbytes, kp.size)
# two batches in flight over RCCL, the second one larger (its buffers grow while the first one's send may still be waiting for its
# peer: no device-wide wait may sit under a lock another shard's first calls need - ADVICE r04), then a third, larger still
g.set_option('gather_wire', 1)
grow = [np.stack([synth_frame(320, 240, 900 + 16 * b + i) for i in range(2 * 3 ** b)]) for b in range(3)]      # 2, 6, 18 frames
got = []
g.submit(grow[0], params)
for b in range(1, len(grow) + 1):
    if b < len(grow):
        g.submit(grow[b], params)
    g.collect()
    got.append((g.counts().copy(),) + tuple(a.copy() for a in g.results()))
for b, (counts, kp, desc) in zip(grow, got):
    c.calculate_batch(b, params)
    wkp, wdesc = c.results()
    assert counts.tolist() == c.counts().tolist()
    assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
g.close(); c.close()
print('rccl loopback ok:', why)
"""


def test_group_gather_over_rccl_on_one_gpu(ctx):
    """The native RCCL gather of sift_hip_group on a box with one GPU: a group of one shard with option gather_loopback sends its
    packed lists (and, with gather_wire = 0, its plain arrays) through ncclSend / ncclRecv to the same rank - communicator from
    ncclCommInitAll, grouped point-to-point, arrival area, unpack - and returns the single context's results; then submit, submit,
    collect with batches that grow (2, 6, 18 frames) over the same communicator."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GROUP_RCCL_SCRIPT.format(root=root)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rccl loopback ok" in r.stdout, r.stdout + r.stderr[-3000:]


def test_cpp_multi_gpu_example(ctx, tmp_path):
    """examples/sift_multi_gpu.cpp: the group API from C++ (two shards on this box's GPU), checked frame by frame against
    sift::Sift inside the program."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sift_multi_gpu"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_multi_gpu.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-L/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    # one attempt: a run that dies (rounds 2 - 4: inside the HIP runtime's per-launch lookup, which the library no longer uses) or
    # ends with a wrong answer (exit status 2) or any other status fails the test
    out = _run_past_runtime_crashes([str(exe), os.path.join(root, "tests", "golden", "parrot_r.pgm"), "5", "2"], cwd=tmp_path, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok: 5 frames over 2 shards"), out.stdout + out.stderr


def test_cpp_multi_gpu_example_soak(ctx, tmp_path):
    """examples/sift_multi_gpu.cpp 25 times in a row (three host threads launching on one GPU + the gather thread): every run
    ends with the right answer, none dies.  (Until round 4 up to 20 of the 25 runs were allowed to die inside the HIP runtime's
    per-launch lookup of the kernel's host stub; the library no longer goes through it: launch_cache.h,
    profiles/r05_launch_ab_soak.txt - 0 of 300 against 13 of 300.)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sift_multi_gpu"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sift_multi_gpu.cpp"), "-L" + os.path.join(root, "sift_amd", "lib"),
                           "-lsift_hip", "-Wl,-rpath," + os.path.join(root, "sift_amd", "lib"), "-L/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    failed = []
    for i in range(25):
        out = subprocess.run([str(exe), os.path.join(root, "tests", "golden", "parrot_r.pgm"), "5", "2"], cwd=tmp_path,
                             capture_output=True, text=True, timeout=300)
        if out.returncode != 0 or not out.stdout.startswith("ok: 5 frames over 2 shards"):
            failed.append((i, out.returncode, out.stdout[-300:], out.stderr[-300:]))
    assert not failed, failed


def test_cli_result_file(ctx, tmp_path, monkeypatch):
    """sift_amd.cli (main.cpp's options, ingest, result writer and overlay): whole result file and overlay."""
    from sift_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    import shutil
    shutil.copy(os.path.join(root, "tests", "golden", "parrot_r.pgm"), tmp_path / "parrot_r.pgm")
    assert cli.main(["-i", "parrot_r.pgm", "-o", "4", "-d", "3", "-r", "1"]) == 0
    want, run = expected_result_file(tmp_path, read_pgm(os.path.join(root, "tests", "golden", "parrot_r.pgm")), 3, 4)
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want
    check_overlay(tmp_path / "parrot_r.pgm_orientation.png", cli.read_image_bgr("parrot_r.pgm"), run, False)
    # the reference's defaults (main.cpp:33-38: sigma 1.6, k sqrt2, 4 octaves, 3 DoGs, no subpixel, no result file), positional image
    os.remove(tmp_path / "interstpoints.txt")
    assert cli.main(["parrot_r.pgm", "--no-overlay"]) == 0 and not os.path.exists(tmp_path / "interstpoints.txt")


def test_cli_reads_a_jpeg(ctx, tmp_path, monkeypatch):
    """The reference's example input is a JPEG (example/parrot.jpg): the command line program decodes one itself
    (sift_amd/csrc/jpeg_decode.cpp, no libjpeg, no PIL), takes its red band (App. B-15) and draws on its B,G,R pixels."""
    from sift_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    import shutil
    shutil.copy(os.path.join(root, "tests", "golden", "img", "scene_420.jpg"), tmp_path / "scene.jpg")
    exp = np.load(os.path.join(root, "tests", "golden", "img", "expected_jpeg.npz"))
    assert cli.main(["-i", "scene.jpg", "-o", "4", "-d", "3", "-r", "1"]) == 0
    want, run = expected_result_file(tmp_path, exp["scene_420.jpg/band0"], 3, 4)
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want and len(want) > 10000
    check_overlay(tmp_path / "scene.jpg_orientation.png", exp["scene_420.jpg/bgr"], run, False)


def test_config3_exception_and_nearest_runnable(ctx, report_dir):
    """BASELINE config 3: 1920x1080, subpixel, 4 oct x 5 DoG throws in the reference (App. B-13);
    the nearest runnable setting (subpixel, 4 x 3) is compared in full."""
    img = synth_frame(1920, 1080, 7)
    run = O.OracleRun(np.zeros_like(img), 5, 4, subpixel=True)
    assert run.status == 1 and "separableConvolveY(): kernel longer than line" in run.error
    with pytest.raises(PreconditionViolation) as e:
        ctx.calculate_batch(img[None], _lib.Params(5, 4, 1.6, O.K_SQRT2, 1))
    assert str(e.value) == run.error
    im = ctx.image(0)                              # the caller's image was already replaced (B-16)
    assert im is not None and im.shape == (2160, 3840)
    # the nearest runnable setting at FULL size: every level of the 3840x2160-base pyramid, every stage list, descriptors
    rep = compare_run(ctx, img, 3, 4, True, "config3 1920x1080 subpixel 4x3", report_dir)
    assert rep["final"] > 5000


def test_config5_batch_of_eight_4k_frames(ctx):
    """BASELINE config 5's per-GPU share (64 frames over 8 GPUs = 8 per GPU): a batch of eight 3840x2160 frames, subpixel
    (7680x4320 base), 5 octaves (6 throw, App. B-14).  First and last frame of the batch are the digest frame
    (tests/golden/digest_config5_4k.npz, oracle): stage counts and SHA-256 of keypoints, orientations, scales and
    descriptors per image; the frames in between are different images (sift.cpp:37-54 runs per image)."""
    from golden_util import GOLDEN
    g = np.load(os.path.join(GOLDEN, "digest_config5_4k.npz"))
    dogs, octaves, subpixel, w, h, seed = (int(v) for v in g["meta"])
    frames = np.stack([synth_frame(w, h, s) for s in (seed, 21, 22, 23, 24, 25, 26, seed)])
    ctx.calculate_batch(frames, _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, subpixel))
    counts = ctx.counts()
    assert counts.size == 8 and (ctx.status() == 0).all()
    kp, desc = ctx.results()
    base = np.concatenate([[0], np.cumsum(counts)])
    for image in (0, 7):
        got = [ctx.stage(s, image).size for s in ("candidates", "after_sort1", "after_orient", "after_sort2", "final")]
        assert got == g["counts"].tolist(), image
        k, d = kp[base[image]:base[image + 1]], desc[base[image]:base[image + 1]]
        assert sha(np.stack([k["x"], k["y"], k["octave"], k["index"]], 1).astype(np.uint16)) == str(g["kp_sha"])
        assert sha(k["orientation"]) == str(g["orientation_sha"]) and sha(k["scale"]) == str(g["scale_sha"])
        assert sha(d) == str(g["descriptors_sha"])
    assert len(set(counts[1:7].tolist())) > 1 and counts[1] != counts[0]     # the other frames are other images


def _gather_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from sift_amd.gather import device_results, gather_finish, gather_start, split_records, unpack_sparse
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    c = Context(0)
    frames = np.stack([synth_frame(320, 240, 10 * rank + i + 1) for i in range(2)])
    c.calculate_batch(frames, _lib.Params(3, 3, 1.6, O.K_SQRT2, 0))
    kp, desc = device_results(c, c.total(), dev, wire="sparse")
    h = gather_start(kp.cpu(), desc.cpu(), torch.from_numpy(c.counts()), dst=0, floats_per_kp=None, bytes_per_kp=34)
    res = gather_finish(h)
    if rank == 0:
        recs, masks = split_records(res[0])
        q.put((recs.numpy().copy(), unpack_sparse(masks, res[1]).numpy().copy(), res[2].numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_of_device_results_two_ranks_sharing_the_gpu(ctx):
    """The N > 1 path of bench.py end to end on real results: in-place views of the library's result arrays,
    the sparse wire format (packed on the GPU), the gather (gloo, because both ranks have to share this box's one GPU)."""
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    kp_all, desc_all, counts_all = q.get(timeout=300)
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    frames = np.stack([synth_frame(320, 240, s) for s in (1, 2, 11, 12)])   # rank 0's frames, then rank 1's
    ctx.calculate_batch(frames, _lib.Params(3, 3, 1.6, O.K_SQRT2, 0))
    kp, desc = ctx.results()
    assert counts_all.tolist() == ctx.counts().tolist()
    assert kp_all.tobytes() == kp.tobytes()
    assert desc_all.tobytes() == desc.tobytes()


def _rccl_loopback_worker(port, q):
    """One process, one GPU, a real RCCL communicator: the gather's messages (header | records, values; device memory,
    sparse wire format packed by the library) go through RCCL's point-to-point path to this same rank."""
    import torch
    import torch.distributed as dist
    from sift_amd.gather import KeypointGather, device_results, split_records, unpack_sparse
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    c = Context(0)
    c.set_option("wire_count", 1)       # as bench.py does for N > 1: the descriptor kernel counts the wire floats itself
    g = KeypointGather(2, dev, loopback=True)
    batches = [np.stack([synth_frame(320, 240, 31), synth_frame(320, 240, 32)]),
               np.stack([np.full((240, 320), 7.0, np.float32)] * 2),                       # a step without a single keypoint
               np.stack([synth_frame(320, 240, 33), np.full((240, 320), 9.0, np.float32)]),
               np.stack([synth_frame(320, 240, 34), synth_frame(320, 240, 35)])]
    want, done = [], []
    for b in batches:
        c.calculate_batch(b, _lib.Params(3, 3, 1.6, O.K_SQRT2, 0))
        kp, desc = c.results()
        want.append((c.counts().copy(), kp.copy(), desc.copy()))
        rec, val = device_results(c, c.total(), dev, wire="sparse", rec_out=g.records_buffer(c.total() * 34))
        done += g.push(rec, val, c.counts())
    done += g.flush()
    dist.barrier()
    torch.cuda.synchronize()
    out = []
    for rec_all, val_all, counts in done:
        recs, masks = split_records(rec_all.cpu())
        out.append((counts.cpu().numpy().copy(), recs.numpy().copy(), unpack_sparse(masks, val_all.cpu()).numpy().copy()))
    q.put((want, out, g.wire_bytes))
    dist.destroy_process_group()


def test_keypoint_gather_over_rccl_on_one_gpu(ctx):
    """RCCL itself, on the one GPU this box has: the lagged-header gather of bench.py's N > 1 path with every message sent through
    RCCL point-to-point to the same rank (world of one process, KeypointGather(loopback=True)) — device tensors, the exact
    message shapes and sizes of the multi-GPU run, zero-keypoint steps included; what arrives equals what the context returned."""
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    p = mpc.Process(target=_rccl_loopback_worker, args=(port, q))
    p.start()
    want, out, wire = q.get(timeout=300)
    p.join(120)
    assert p.exitcode == 0
    assert len(out) == len(want) == 4
    total = 0
    for (wc, wk, wd), (gc, gk, gd) in zip(want, out):
        assert gc.tolist() == wc.tolist()
        assert gk.tobytes() == wk.tobytes() and gd.tobytes() == wd.tobytes()
        total += int(wc.sum())
    assert total > 500 and wire > 34 * total


def test_batch_pipeline_matches_single_context(ctx):
    """Batches in flight on a ring of contexts (sift_amd/pipeline.py) give, batch for batch, the single context's results."""
    from sift_amd.pipeline import BatchPipeline
    params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    batches = [np.stack([synth_frame(480, 360, 100 + 4 * b + i) for i in range(4)]) for b in range(5)]
    got = []
    with BatchPipeline(0, depth=2) as pipe:
        tickets = []
        for b in batches:
            tickets.append(pipe.submit(b, params))
            if len(tickets) == 2:
                t = tickets.pop(0)
                c = t.result()
                got.append((c.counts().copy(),) + tuple(a.copy() for a in c.results()))
                t.release()
        with pytest.raises(RuntimeError):   # both slots taken: the third submit must be refused, not overwrite results
            pipe.submit(batches[0], params)
            pipe.submit(batches[0], params)
        for t in tickets:
            c = t.result()
            got.append((c.counts().copy(),) + tuple(a.copy() for a in c.results()))
            t.release()
    assert len(got) == len(batches)
    for b, (counts, kp, desc) in zip(batches, got):
        ctx.calculate_batch(b, params)
        wkp, wdesc = ctx.results()
        assert counts.tolist() == ctx.counts().tolist() and counts.sum() > 0
        assert kp.tobytes() == wkp.tobytes()
        assert desc.tobytes() == wdesc.tobytes()


def test_library_before_torch_in_one_process(tmp_path):
    """libsift_hip loaded and used BEFORE torch initialises its GPU runtime: both must see the GPU (one HIP
    runtime per process, sift_amd/_lib.py:_preload_hip_runtime)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {root!r})\n"
        "from sift_amd import _lib\n"
        "from sift_amd.sift import Context\n"
        "from sift_amd.synthetic import synth_frame\n"
        "c = Context(0)\n"
        "c.calculate_batch(synth_frame(200, 160, 2)[None], _lib.Params(3, 2, 1.6, 2 ** 0.5, 0))\n"
        "n = c.total()\n"
        "import torch\n"
        "assert torch.cuda.is_available(), 'torch lost the GPU'\n"
        "t = torch.arange(8, device='cuda:0').sum().item()\n"
        "c.calculate_batch(synth_frame(200, 160, 2)[None], _lib.Params(3, 2, 1.6, 2 ** 0.5, 0))\n"
        "assert c.total() == n and n > 0 and t == 28\n"
        "print('ok', n)\n"
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("gated", [True, False], ids=["gated", "ungated"])
def test_batch_pipeline_survives_a_failing_batch(ctx, gated):
    """A batch that ends in the reference's exception (pyramid level smaller than the blur kernel, App. B-13; or the
    dead 16x16 blur, B-14, which only shows after the cleanup) releases what it owes the phase gate: its neighbours in
    the pipeline complete with the single context's results, the failing tickets raise."""
    from sift_amd.pipeline import BatchPipeline
    good = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    plan_fail = _lib.Params(3, 4, 1.6, O.K_SQRT2, 0)     # 160x120, 4 octaves: fails when the plan is built
    late_fail = _lib.Params(4, 3, 1.6, O.K_SQRT2, 0)     # 512x384, 4 DoGs: fails in the orientation stage, if at all
    frames = [np.stack([synth_frame(160, 120, 200 + 2 * b + i) for i in range(2)]) for b in range(6)]
    big = synth_frame(512, 384, 3)[None]
    jobs = [(frames[0], good), (frames[1], plan_fail), (frames[2], good), (big, late_fail), (frames[4], good), (frames[5], good)]
    out = []
    with BatchPipeline(0, depth=2, gated=gated) as pipe:
        tickets = []

        def collect(t):
            try:
                c = t.result()
                out.append((c.counts().copy(),) + tuple(a.copy() for a in c.results()))
            except PreconditionViolation as e:
                out.append(e)
            t.release()

        for imgs, prm in jobs:
            tickets.append(pipe.submit(imgs, prm))
            if len(tickets) == 2:
                collect(tickets.pop(0))
        for t in tickets:
            collect(t)
    assert len(out) == len(jobs)
    for (imgs, prm), got in zip(jobs, out):
        try:
            ctx.calculate_batch(imgs, prm)
            want = (ctx.counts().copy(),) + tuple(a.copy() for a in ctx.results())
        except PreconditionViolation as e:
            assert isinstance(got, PreconditionViolation) and str(got) == str(e)
            continue
        assert not isinstance(got, Exception), got
        assert got[0].tolist() == want[0].tolist()
        assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert isinstance(out[1], PreconditionViolation) and not isinstance(out[0], Exception) and not isinstance(out[5], Exception)


def test_batch_pipeline_run_stream(ctx):
    """BatchPipeline.run_stream: every context's host thread takes its next batch from the source itself and hands its results
    to the sink before the next one (no dispatching thread in between).  Nine different batches through two gated contexts: each
    batch's results are those of the single context; a source that raises, or a batch that ends in the reference's exception,
    ends the stream with that exception after the batches in flight are done."""
    from sift_amd.pipeline import BatchPipeline
    prm = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    batches = [np.stack([synth_frame(320, 240, 300 + 3 * b + i) for i in range(3)]) for b in range(9)]
    got = {}
    with BatchPipeline(0, depth=2) as pipe:
        it = iter(range(len(batches)))

        order = []

        def source_tagged():
            b = next(it, None)
            if b is None:
                return None
            order.append(b)
            return (batches[b], prm)

        def sink(c, slot, item):
            b = next(i for i, a in enumerate(batches) if a is item[0])
            got[b] = (slot, c.counts().copy()) + tuple(a.copy() for a in c.results())

        pipe.run_stream(source_tagged, sink)
        assert order == list(range(9)) and sorted(got) == list(range(9))
        assert {got[b][0] for b in got} == {0, 1}, "both contexts should have taken batches"
        # a failing batch ends the stream with the reference's exception
        bad = _lib.Params(3, 4, 1.6, O.K_SQRT2, 0)   # 160x120, 4 octaves: a pyramid level shorter than the blur kernel's radius (App. B-13)
        small = np.stack([synth_frame(160, 120, 400 + i) for i in range(2)])
        jobs = iter([(batches[0], prm), (small, bad), (batches[2], prm), (batches[3], prm)])
        with pytest.raises(PreconditionViolation):
            pipe.run_stream(lambda: next(jobs, None), None)
        # ... and the pipeline is usable afterwards
        t = pipe.submit(batches[4], prm)
        assert t.result().counts().tolist() == got[4][1].tolist()
        t.release()
    for b in range(9):
        ctx.calculate_batch(batches[b], prm)
        assert got[b][1].tolist() == ctx.counts().tolist()
        kp, desc = ctx.results()
        assert got[b][2].tobytes() == kp.tobytes() and got[b][3].tobytes() == desc.tobytes()


def check_sparse_wire_kernels(ctx, frames, params):
    """sift_hip_result_sparse_size / _pack / sift_hip_sparse_unpack on the results of `frames` under `params` against the torch
    restatement of the wire format (sift_amd/gather.py:pack_sparse), with the counting pass on its own and (option wire_count)
    riding in the descriptor kernel.  -> (keypoint records, descriptors)."""
    import torch
    from sift_amd.gather import device_results, join_records, pack_sparse, split_records, unpack_sparse
    ctx.calculate_batch(frames, params)
    kp, desc = ctx.results()
    total = ctx.total()
    assert total > 0
    rec, values = device_results(ctx, total, torch.device("cuda", 0), wire="sparse")
    masks_ref, values_ref = pack_sparse(torch.from_numpy(desc.reshape(-1)))
    rec_ref = join_records(torch.from_numpy(kp.view(np.uint8).reshape(-1)), masks_ref)
    assert values.numel() == values_ref.numel() == ctx.sparse_size()
    assert rec.cpu().numpy().tobytes() == rec_ref.numpy().tobytes()
    assert values.cpu().numpy().tobytes() == values_ref.numpy().tobytes()
    recs, masks = split_records(rec.cpu())
    assert recs.numpy().tobytes() == kp.tobytes()
    assert unpack_sparse(masks, values.cpu()).numpy().tobytes() == desc.tobytes()
    # the receiving side on the GPU (sift_hip_sparse_unpack): the same records and descriptors, bit for bit
    kp_dev = torch.full((total * 20,), 0xAB, dtype=torch.uint8, device="cuda:0")
    desc_dev = torch.full((total * 128,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sparse_unpack(rec.data_ptr(), values.data_ptr(), total, kp_dev.data_ptr(), desc_dev.data_ptr())
    assert kp_dev.cpu().numpy().tobytes() == kp.tobytes() and desc_dev.cpu().numpy().tobytes() == desc.tobytes()
    assert 0.2 < values.numel() / (total * 112) < 0.6   # the saving the format exists for
    # option wire_count: the counting pass rides in the descriptor kernel (what bench.py uses for N > 1); same wire bytes
    ctx.set_option("wire_count", 1)
    try:
        ctx.calculate_batch(frames, params)
        assert ctx.sparse_size() == values_ref.numel()
        rec2, values2 = device_results(ctx, total, torch.device("cuda", 0), wire="sparse")
        assert rec2.cpu().numpy().tobytes() == rec_ref.numpy().tobytes() and values2.cpu().numpy().tobytes() == values_ref.numpy().tobytes()
    finally:
        ctx.set_option("wire_count", 0)
    return kp, desc


def test_sparse_wire_kernels_match_the_reference_packing(ctx):
    """sift_hip_result_sparse_size / _pack (kernels_wire.hip) against the torch restatement of the wire format
    (sift_amd/gather.py:pack_sparse) on real results, and the round trip back to the 128-float descriptors."""
    frames = np.stack([synth_frame(640, 480, 30 + i) for i in range(3)] + [np.full((480, 640), 7.0, np.float32)])   # last: no keypoints
    check_sparse_wire_kernels(ctx, frames, _lib.Params(3, 3, 1.6, O.K_SQRT2, 0))
    assert ctx.counts()[-1] == 0


def test_deferred_sparse_pack_survives_the_next_batch(ctx):
    """sift_hip_result_sparse_pack_async only QUEUES the pack (side stream) and lets the context start its next batch at once
    (what bench.py's N > 1 loop does): the lists packed from batch A must be A's, bit for bit, although batch B - other frames,
    other keypoints - rewrites the context's arrays right behind the call; sift_hip_result_pack_wait may come from another
    thread."""
    import threading
    import torch
    from sift_amd.gather import device_results
    params = _lib.Params(3, 3, 1.6, O.K_SQRT2, 0)
    frames_a = np.stack([synth_frame(640, 480, 50 + i) for i in range(4)])
    frames_b = np.stack([synth_frame(640, 480, 90 + i) for i in range(4)])
    dev = torch.device("cuda", 0)
    ctx.set_option("wire_count", 1)
    try:
        ctx.calculate_batch(frames_b, params)
        total_b = ctx.total()
        rec_b, val_b = device_results(ctx, total_b, dev, wire="sparse")
        ctx.calculate_batch(frames_a, params)
        total_a = ctx.total()
        rec_a, val_a = device_results(ctx, total_a, dev, wire="sparse")          # the synchronous pack: the expectation
        assert total_a != total_b or rec_a.cpu().numpy().tobytes() != rec_b.cpu().numpy().tobytes()
        for round_ in range(6):
            ctx.calculate_batch(frames_a, params)
            rec, val = device_results(ctx, total_a, dev, wire="sparse", defer_pack=True)
            ctx.calculate_batch(frames_b, params)                                   # no wait in between
            waiter = threading.Thread(target=ctx.pack_wait)
            waiter.start()
            waiter.join()
            assert rec.cpu().numpy().tobytes() == rec_a.cpu().numpy().tobytes(), round_
            assert val.cpu().numpy().tobytes() == val_a.cpu().numpy().tobytes(), round_
            assert ctx.total() == total_b
            rec2, val2 = device_results(ctx, total_b, dev, wire="sparse")
            assert rec2.cpu().numpy().tobytes() == rec_b.cpu().numpy().tobytes() and val2.cpu().numpy().tobytes() == val_b.cpu().numpy().tobytes()
        ctx.pack_wait()      # nothing pending: returns at once
    finally:
        ctx.set_option("wire_count", 0)


# ------------------------------------------------------------------------------------------------
# the HIP path against what the reference's own prebuilt binary returned (tests/golden/refpin.npz, see
# tests/test_ref_pins.py): no oracle in between
# ------------------------------------------------------------------------------------------------
import make_ref_pins as REFPIN  # noqa: E402  (tests/golden is put on the path by conftest.py)


def _refpin():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin.npz"))


@pytest.mark.parametrize("name", sorted(REFPIN.CALC_CASES))
def test_hip_matches_the_reference_binary(ctx, name):
    hip_against_pin(ctx, _refpin(), REFPIN.CALC_CASES, name)


@pytest.mark.parametrize("name", sorted(REFPIN.HARD_CASES))
def test_hip_matches_the_reference_binary_on_hard_frames(ctx, name):
    """tests/hard_frames.py's content (refpin_hard_frames.npz): several records per keypoint with the first peak twice, NaN
    orientations - a NaN equals a NaN, the x86 default NaN's sign bit is not the GPU's -, all-zero descriptors, plateaus,
    mirror symmetry."""
    hip_against_pin(ctx, np.load(REFPIN.HARD_PIN), REFPIN.HARD_CASES, name, nan_equals_nan=True)
    if name.startswith("signed"):
        assert ctx.stage("after_orient").size > ctx.stage("after_sort1").size      # the batch was redone by mid_host


def hip_against_pin(ctx, pin, cases, name, nan_equals_nan=False):
    import hashlib
    import re
    spec, dogs, octaves, sub = cases[name][:4]
    sigma, k = cases[name][4:] if len(cases[name]) > 4 else (1.6, O.K_SQRT2)      # (REFPIN.SCALE_CASES carry their own)
    img = REFPIN.make_image(spec)
    assert sha(img) == str(pin[f"calc/{name}/image_sha"])
    params = _lib.Params(dogs, octaves, sigma, k, sub)
    if f"calc/{name}/exception" in pin.files:
        with pytest.raises(PreconditionViolation) as e:
            ctx.calculate_batch(img[None], params)
        want = re.sub(r"\n\(/[^)]*\)\n+$", "\n", str(pin[f"calc/{name}/exception"]).lstrip("\n"))   # Vigra's what() minus (header:line)
        assert str(e.value).strip() == want.strip()
        return
    ctx.calculate_batch(img[None], params)
    ref = pin[f"calc/{name}/points"]
    kp, desc = ctx.results()
    assert kp.size == ref.size
    for f in ("x", "y", "octave", "index"):
        assert (kp[f] == ref[f]).all(), f
    assert kp["scale"].tobytes() == ref["scale"].tobytes()
    if nan_equals_nan:
        assert_bits_equal(kp["orientation"], ref["orientation"], f"{name}: orientation")
    else:
        assert kp["orientation"].tobytes() == ref["orientation"].tobytes()
    assert (kp["has_descriptor"].astype(bool) == (ref["n_desc"] == 128)).all()
    d = desc[kp["has_descriptor"].astype(bool)].reshape(-1)
    assert hashlib.sha256(d.tobytes()).hexdigest() == str(pin[f"calc/{name}/desc_sha"])
    mw, mh = (int(v) for v in pin[f"calc/{name}/levels_wh"])
    for o in range(mw):
        for j in range(mh):
            k = o * mh + j
            lv = ctx.level("gaussian", o, j, 0)
            assert tuple(pin[f"calc/{name}/level_dims"][k]) == (lv.shape[1], lv.shape[0])
            assert np.float32(ctx.level_scale("gaussian", o, j)).view(np.uint32) == pin[f"calc/{name}/level_scale_bits"][k]
            assert sha(lv) == str(pin[f"calc/{name}/level_sha"][k]), f"gaussian({o},{j})"
    dw, dh = (int(v) for v in pin[f"calc/{name}/dogs_wh"])
    for o in range(dw if not sub else 0):   # (the stand-alone _createDOGs call of the pin saw the raw frame)
        for j in range(dh):
            k = o * dh + j
            lv = ctx.level("dog", o, j, 0)
            assert np.float32(ctx.level_scale("dog", o, j)).view(np.uint32) == pin[f"calc/{name}/dog_scale_bits"][k]
            assert sha(lv) == str(pin[f"calc/{name}/dog_sha"][k]), f"dog({o},{j})"
    w, h = (int(v) for v in pin[f"calc/{name}/image_dims"])
    if sub:   # the caller's image was replaced by the 2x frame (sift.cpp:20-21)
        assert ctx.image(0).shape == (h, w)
    else:
        assert img.shape == (h, w)


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_bench_frame.npz")),
                    reason="fixture not generated")
def test_hip_bench_frame_matches_the_reference_binary(ctx):
    """Frame 1 of the bench workload (1920x1080, 3 DoGs x 4 octaves) against what the reference binary returned for it."""
    import hashlib
    pin = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_bench_frame.npz"))
    img = synth_frame(1920, 1080, 1)
    assert sha(img) == str(pin["image_sha"])
    ctx.calculate_batch(img[None], _lib.Params(3, 4, 1.6, O.K_SQRT2, 0))
    kp, desc = ctx.results()
    ref = pin["points"]
    assert kp.size == ref.size
    for f in ("x", "y", "octave", "index"):
        assert (kp[f] == ref[f]).all(), f
    assert kp["scale"].tobytes() == ref["scale"].tobytes() and kp["orientation"].tobytes() == ref["orientation"].tobytes()
    assert hashlib.sha256(desc[kp["has_descriptor"].astype(bool)].tobytes()).hexdigest() == str(pin["desc_sha"])
    mw, mh = (int(v) for v in pin["levels_wh"])
    for o in range(mw):
        for j in range(mh):
            assert sha(ctx.level("gaussian", o, j, 0)) == str(pin["level_sha"][o * mh + j]), f"gaussian({o},{j})"


def test_hip_config2_as_written_matches_the_reference_binary(ctx):
    """BASELINE.json configs[1] exactly as written (one 640x480 frame, seed 1, 4 octaves x 3 DoGs) against what the reference's
    own binary returned for it: keypoints, scales, orientations, descriptors, every Gaussian and DoG level - no oracle in between."""
    import hashlib
    pin = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_config2.npz"))
    img = synth_frame(640, 480, 1)
    assert sha(img) == str(pin["image_sha"])
    ctx.calculate_batch(img[None], _lib.Params(3, 4, 1.6, O.K_SQRT2, 0))
    kp, desc = ctx.results()
    ref = pin["points"]
    assert kp.size == ref.size
    for f in ("x", "y", "octave", "index"):
        assert (kp[f] == ref[f]).all(), f
    assert kp["scale"].tobytes() == ref["scale"].tobytes() and kp["orientation"].tobytes() == ref["orientation"].tobytes()
    assert hashlib.sha256(desc[kp["has_descriptor"].astype(bool)].tobytes()).hexdigest() == str(pin["desc_sha"])
    mw, mh = (int(v) for v in pin["levels_wh"])
    for o in range(mw):
        for j in range(mh):
            assert sha(ctx.level("gaussian", o, j, 0)) == str(pin["level_sha"][o * mh + j]), f"gaussian({o},{j})"
    dw, dh = (int(v) for v in pin["dogs_wh"])
    for o in range(dw):
        for j in range(dh):
            assert sha(ctx.level("dog", o, j, 0)) == str(pin["dog_sha"][o * dh + j]), f"dog({o},{j})"


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_u16_truncation.npz")),
                    reason="fixture not generated")
def test_hip_u16_truncation_matches_the_reference_binary(ctx):
    """App. B-7 against the reference binary itself: 66260 survivors of the first cleanup on a 1024x1088 blob lattice,
    `u16_t size` (sift.cpp:41) keeps 724 of them, 720 are returned; keypoints, orientations and descriptors bit for bit."""
    from sift_amd.synthetic import blob_frame
    pin = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_u16_truncation.npz"))
    w, h, seed = (int(v) for v in pin["params"][3:6])
    img = blob_frame(w, h, seed)
    assert sha(img) == str(pin["image_sha"]) and int(pin["rc"]) == 0
    ctx.calculate_batch(img[None], _lib.Params(3, 4, 1.6, O.K_SQRT2, 0))
    assert ctx.stage("after_sort1").size == 724
    kp, desc = ctx.results()
    ref = pin["points"]
    assert kp.size == ref.size == 720
    for f in ("x", "y", "octave", "index"):
        assert (kp[f] == ref[f]).all(), f
    assert kp["scale"].tobytes() == ref["scale"].tobytes() and kp["orientation"].tobytes() == ref["orientation"].tobytes()
    assert desc[kp["has_descriptor"].astype(bool)].reshape(-1).tobytes() == pin["desc"].tobytes()


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_configs_as_written.npz")),
                    reason="fixture not generated")
@pytest.mark.parametrize("name", ["config3_as_written", "config5_octave5_1792"])
def test_hip_baseline_configs_as_written_end_like_in_the_reference_binary(ctx, name):
    """BASELINE.json configs[2] exactly as written, and configs[4]'s failure mode (the dead 16x16 blur of an octave-5 keypoint) on
    the 1792x1792 six-octave frame the reference binary was run on (tests/golden/make_ref_pins.py config5): the binary throws;
    so does the HIP path, with the same text."""
    import re
    pin = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_configs_as_written.npz"))
    if name + "/rc" not in pin.files:
        pytest.skip("case not in the fixture")
    dogs, octaves, sub, w, h, seed = (int(v) for v in pin[name + "/params"])
    so = str(pin[name + "/stdout"])
    assert int(pin[name + "/rc"]) == 5 and so.startswith("EXCEPTION ")
    with pytest.raises(PreconditionViolation) as e:
        ctx.calculate_batch(synth_frame(w, h, seed)[None], _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, sub))
    want = re.sub(r"\n\(/[^)]*\)\n+$", "\n", so[len("EXCEPTION "):].lstrip("\n"))
    assert str(e.value).strip() == want.strip()
