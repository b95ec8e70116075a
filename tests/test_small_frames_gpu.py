"""Tiny and thin frames on the GPU: levels barely longer than the largest blur radius, against the CPU oracle bit for bit.

The rows of tests/small_frames.py (tests/test_small_frames_host.py pins what the oracle makes of them) put almost every kernel
where no other test takes it: both halos of a blur tile or strip outside the image at once, a reflected halo as long as the
line, halo columns beyond the one reflection vigra allows (they must carry no weight), the streaming / pair / kept-pixels
launchers declining a shape and the generic path running instead, extremum tiles wider and higher than the image, 16x16
descriptor windows that touch both borders, 8-bit batches shorter than a handful of 16-byte vectors, and the precondition's
text at the exact size edge.  Every comparison goes through tests/test_gpu_parity.py's compare_run: every Gaussian and DoG
level, the gradient maps, all five stage lists, orientations, descriptors.
"""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import small_frames as S
from sift_amd import _lib
from sift_amd.sift import PreconditionViolation, Sift
from test_gpu_parity import check_overlay, check_u8_frames_in_sparse_lists_out, compare_run
from test_small_frames_host import BOUNDARY, COUNTS

pytestmark = pytest.mark.gpu

STAGES = ("candidates", "after_sort1", "after_orient", "after_sort2", "final")


def run_row(ctx, report_dir, name, what, frames=1):
    """One row through compare_run; its candidate and final counts must be the oracle's pinned ones; they go to the report."""
    dogs, octaves, sigma, subpixel = S.ROW[name][5:]
    rep = compare_run(ctx, S.row_image(name), dogs, octaves, subpixel, f"{name} [{what}]", report_dir, batch_of=frames, sigma=sigma, run=S.row_run(name))
    assert (rep["candidates"], rep["final"]) == COUNTS[name]
    for image in range(frames):
        assert (ctx.stage("candidates", image).size, ctx.stage("final", image).size) == COUNTS[name]
    with open(os.path.join(report_dir, "small_frames.jsonl"), "a") as f:
        f.write(json.dumps({"row": name, "path": what, "frames": frames, "candidates": rep["candidates"], "final": rep["final"]}) + "\n")
    return rep


@pytest.mark.parametrize("name", S.IDS)
def test_rows_default_path(ctx, report_dir, name):
    run_row(ctx, report_dir, name, "default path")


# stream_min_waves = 1 offers every blur to the streaming kernels, blur_pair / pair_waves the first two levels to the pair kernel,
# three frames the decimating blur of the two-octave rows to the kept-pixels kernel and its own fallbacks.  A launcher that
# declines a shape (too few rows for a chunk, a width that is no multiple of the lane vector) hands it to the generic path:
# that is the behaviour under test, and parity must hold either way.
FORCED = {
    "streaming": (dict(stream_min_waves=1), 1),
    "pair": (dict(blur_pair=1, stream_min_waves=1, pair_waves=64), 1),
    "streaming x3": (dict(stream_min_waves=1), 3),
}


@pytest.mark.parametrize("setting", sorted(FORCED))
@pytest.mark.parametrize("name", S.IDS)
def test_rows_forced_paths(ctx, report_dir, name, setting):
    options, frames = FORCED[setting]
    try:
        for option, value in options.items():
            ctx.set_option(option, value * frames if option == "pair_waves" else value)
        run_row(ctx, report_dir, name, setting, frames=frames)
    finally:
        ctx.set_option("stream_min_waves", 0)
        ctx.set_option("pair_waves", 0)


def assert_image_is_the_runs(ctx, run, image, what):
    """Stage lists, count, keypoint records and descriptors of one image of the batch against its own oracle run."""
    counts = ctx.counts()
    kp, desc = ctx.results()
    base = int(counts[:image].sum())
    for stage in STAGES:
        got, want = ctx.stage(stage, image), run.points(stage)[0]
        assert got.size == want.size, f"{what}: {stage}: {got.size} points vs oracle {want.size}"
        for f in ("x", "y", "octave", "index"):
            assert (got[f] == want[f]).all(), f"{what}: {stage}: field {f}"
        assert got["scale"].tobytes() == want["scale"].tobytes(), f"{what}: {stage}: scale"
        if stage != "after_sort1":
            assert (got["filtered"].astype(bool) == want["filtered"].astype(bool)).all(), f"{what}: {stage}: filtered"
    want, wdesc = run.points("final")
    assert counts[image] == want.size, f"{what}: count"
    recs = kp[base:base + want.size]
    for f in ("x", "y", "octave", "index"):
        assert (recs[f] == want[f]).all(), f"{what}: result field {f}"
    assert recs["scale"].tobytes() == want["scale"].tobytes() and recs["orientation"].tobytes() == want["orientation"].tobytes()
    assert (recs["has_descriptor"] == (want["n_desc"] == 128)).all()
    assert desc[base:base + want.size].tobytes() == wdesc.tobytes(), f"{what}: descriptors"


BATCH_ROWS = ["15x15", "19x257", "61x31 2oct", "2000x18", "blob 17x400"]


@pytest.mark.parametrize("name", BATCH_ROWS)
def test_batches(ctx, report_dir, name):
    """Three copies of a row in one batch, then three DIFFERENT frames of the row's shape (seeds 1, 2, 3), each image against its
    own oracle run."""
    run_row(ctx, report_dir, name, "batch of 3", frames=3)
    gen, w, h, seed, dogs, octaves, sigma, subpixel = S.ROW[name][1:]
    frames = np.stack([gen(w, h, s) for s in (1, 2, 3)])
    ctx.calculate_batch(frames, _lib.Params(dogs, octaves, sigma, O.K_SQRT2, 1 if subpixel else 0))
    assert ctx.n_images() == 3
    for i in range(3):
        run = O.OracleRun(frames[i], dogs, octaves, sigma=sigma, subpixel=subpixel)
        assert run.status == 0, run.error
        assert_image_is_the_runs(ctx, run, i, f"{name} seed {i + 1} at {i}")
    assert len({ctx.stage("candidates", i).size for i in range(3)}) > 1, "the frames should differ in their candidate counts"


@pytest.mark.parametrize("name,n", [("15x15", 5), ("19x257", 5), ("2000x18", 2)])
def test_u8_and_sparse(ctx, name, n):
    """8-bit frames in, sparse lists out (tests/test_gpu_parity.py's check) on batches of a few hundred to a few thousand bytes:
    5 x 225 and 5 x 4883 bytes are no multiple of 16, so the widening kernel's last thread takes its scalar tail, and the 15x15
    batch is 70 vectors and 5 bytes in all.  The float path's counts must be the oracle's, frame by frame (none for 15x15: the
    empty sparse lists)."""
    gen, w, h, seed, dogs, octaves, sigma, subpixel = S.ROW[name][1:]
    frames = np.stack([gen(w, h, s) for s in range(1, n + 1)])
    want = [O.OracleRun(f, dogs, octaves, sigma=sigma).points("final")[0].size for f in frames]
    assert want[0] == COUNTS[name][1]
    if name != "2000x18":
        assert frames.size % 16 != 0
    counts, kp, desc = check_u8_frames_in_sparse_lists_out(ctx, frames, _lib.Params(dogs, octaves, sigma, O.K_SQRT2, 0), sum(want) - 1)
    assert counts.tolist() == want and kp.size == sum(want)


@pytest.mark.parametrize("plan", S.BOUNDARY_PLANS, ids=[f"s{p[0]} {p[1]}x{p[2]}" for p in S.BOUNDARY_PLANS])
def test_boundary_errors(ctx, report_dir, plan):
    """One pixel below the smallest side the oracle accepts the library raises the oracle's text - separableConvolveX() for the
    width, ...Y() for the height, X first when both are too short -, at the smallest side it runs to parity on each axis and on
    both, and a throwing frame leaves nothing behind for the good frame that follows it in the same context."""
    sigma, dogs, octaves = plan
    w, h, long = BOUNDARY[plan]
    b = S.boundary(*plan)
    assert (b["w"], b["h"], b["long"]) == (w, h, long)
    good = "19x257"
    for size, err in (((w - 1, long), b["err_w"]), ((long, h - 1), b["err_h"]), ((w - 1, h - 1), b["err_both"])):
        assert S.oracle_answer(*size, sigma, dogs, octaves) == (1, err)
        with pytest.raises(PreconditionViolation) as e:
            ctx.calculate_batch(S.boundary_frame(*size)[None], _lib.Params(dogs, octaves, sigma, O.K_SQRT2, 0))
        assert str(e.value) == err, (size, str(e.value))
        run_row(ctx, report_dir, good, f"after {size[0]}x{size[1]} threw under s{sigma} {dogs}x{octaves}")
    for size in ((w, long), (long, h), (w, h)):
        rep = compare_run(ctx, S.boundary_frame(*size), dogs, octaves, False, f"boundary {size[0]}x{size[1]} s{sigma} {dogs}x{octaves}", report_dir, sigma=sigma)
        with open(os.path.join(report_dir, "small_frames.jsonl"), "a") as f:
            f.write(json.dumps({"boundary": list(plan), "size": list(size), "candidates": rep["candidates"], "final": rep["final"]}) + "\n")


def write_pgm(path, img):
    u8 = img.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), img)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + u8.tobytes())


def test_python_mirror_and_cli(ctx, tmp_path, monkeypatch):
    """Sift(3, 1).calculate and the command line program (sift_amd.cli: main.cpp's options, ingest and result writer) on a
    19x257 frame: the result file OracleRun.write_result writes; on a 15x15 frame: exit 0 and the header line alone."""
    from sift_amd import cli
    run = S.row_run("19x257")
    run.write_result(tmp_path / "expected.txt")
    want = open(tmp_path / "expected.txt", "rb").read()
    assert want.count(b"\n") == 1 + COUNTS["19x257"][1]
    img = S.row_image("19x257")
    points = Sift(3, 1, context=ctx).calculate(img)
    final, fdesc = run.points("final")
    assert len(points) == final.size == COUNTS["19x257"][1]
    for p, want_p, want_d in zip(points, final, fdesc):
        assert (p.loc, p.octave, p.index) == ((int(want_p["x"]), int(want_p["y"])), int(want_p["octave"]), int(want_p["index"]))
        assert np.float32(p.scale).tobytes() == want_p["scale"].tobytes() and np.float32(p.orientation).tobytes() == want_p["orientation"].tobytes()
        assert np.array(p.descriptors, np.float32).tobytes() == want_d.tobytes()
    cli.write_result(str(tmp_path / "mirror.txt"), points)
    assert open(tmp_path / "mirror.txt", "rb").read() == want
    monkeypatch.chdir(tmp_path)
    write_pgm(tmp_path / "thin.pgm", img)
    assert cli.main(["-i", "thin.pgm", "-o", "1", "-d", "3", "-r", "1"]) == 0
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want
    check_overlay(tmp_path / "thin.pgm_orientation.png", cli.read_image_bgr("thin.pgm"), run, False)
    os.remove(tmp_path / "interstpoints.txt")
    S.row_run("15x15").write_result(tmp_path / "expected_tiny.txt")
    want = open(tmp_path / "expected_tiny.txt", "rb").read()
    assert want == b"Location\tscale\torientation\tdescriptors\n"
    write_pgm(tmp_path / "tiny.pgm", S.row_image("15x15"))
    assert cli.main(["-i", "tiny.pgm", "-o", "1", "-d", "3", "-r", "1"]) == 0
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want
    assert Sift(3, 1, context=ctx).calculate(S.row_image("15x15")) == []
