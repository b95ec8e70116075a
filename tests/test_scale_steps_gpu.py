"""Scale steps other than sqrt(2) on the GPU: plans with several gradient levels, against the CPU oracle bit for bit.

At k = sqrt(2) every keypoint of the suite's fixed cases takes its gradient maps from Gaussian level (0, 0) and Plan::grad_levels
holds one entry.  The rows of tests/test_scale_steps_host.py select two to four levels, so that these run: the second and later
turns of the loops over the plan's gradient levels (one gradient / weighting / descriptor launch per level, descriptor cells of
a level behind those of the levels before it), keypoints of octave o that carry their coordinates into a level of octave 0,
levels other than 0 and 1 on the side stream, an octave's top level that IS a gradient level and so must be written, and the
gradient maps of levels other than (0, 0).  tests/test_scale_steps_host.py asserts on the CPU that every row populates the
levels listed; every test here asserts it again from what the library returned.
"""
import json
import os

import numpy as np
import pytest

import make_ref_pins as REFPIN
import oracle_lib as O
from sift_amd import _lib
from sift_amd.sift import Sift
from sift_amd.synthetic import synth_frame
from test_gpu_parity import (assert_bits_equal, check_sparse_wire_kernels, check_u8_frames_in_sparse_lists_out, compare_image, compare_run,
                             hip_against_pin)
from test_scale_steps_host import K_EDGES, ROWS, edge_run, populations, row_image, row_run

pytestmark = pytest.mark.gpu

STAGES = ("candidates", "after_sort1", "after_orient", "after_sort2", "final")
R200, R240, R322 = "200x150 3x3 s1.0 k1.8", "240x180 4x3 s0.8 k1.5", "322x250 3x4 s1.0 k1.6"
P18 = (3, 3, 1.0, 1.8)      # dogs, octaves, sigma, k of the 200x150 row: levels (0,0), (0,2) and octave 0's top level (0,3)


def run_row(ctx, report_dir, name, what, frames=1):
    """One row through compare_run - every Gaussian and DoG level, the gradient maps, every stage list, records, descriptors -,
    then the levels the LIBRARY's final keypoints populate, which must be the row's, keypoint for keypoint; they go to the report."""
    dogs, octaves, sigma, k, subpixel, final, levels = ROWS[name][4:]
    rep = compare_run(ctx, row_image(name), dogs, octaves, subpixel, f"{name} [{what}]", report_dir, batch_of=frames, sigma=sigma, k=k, run=row_run(name))
    assert rep["final"] == final
    assert sorted(tuple(l) for l in rep["gradient_levels"]) == sorted(levels) and rep["gradient_levels_unselected"] == []
    for image in sorted({0, frames - 1}):
        got = populations(ctx.stage("final", image), dogs, octaves, sigma, k)
        assert got == levels and len(got) >= 2, f"{name} [{what}] img{image}: levels populated {got}, expected {levels}"
    with open(os.path.join(report_dir, "scale_steps.jsonl"), "a") as f:
        f.write(json.dumps({"row": name, "path": what, "frames": frames, "final": rep["final"],
                            "levels": {f"({o},{j})": n for (o, j), n in sorted(got.items())}}) + "\n")
    return rep


@pytest.mark.parametrize("name", sorted(ROWS))
def test_many_gradient_levels(ctx, report_dir, name):
    run_row(ctx, report_dir, name, "default path")


@pytest.mark.parametrize("name", [R200, R240, R322])
def test_many_gradient_levels_streaming_blur(ctx, report_dir, name):
    ctx.set_option("stream_min_waves", 1)
    try:
        run_row(ctx, report_dir, name, "stream_min_waves=1", frames=2)
    finally:
        ctx.set_option("stream_min_waves", 0)


def test_many_gradient_levels_first_two_levels_in_one_launch(ctx, report_dir):
    frames = 2
    ctx.set_option("blur_pair", 1)
    ctx.set_option("stream_min_waves", 1)
    ctx.set_option("pair_waves", 64 * frames)
    try:
        run_row(ctx, report_dir, R240, "blur_pair, pair_waves=128", frames=frames)
    finally:
        ctx.set_option("stream_min_waves", 0)
        ctx.set_option("pair_waves", 0)


def test_many_gradient_levels_general_orientation_bins(ctx, report_dir):
    ctx.set_option("orient_general", 1)
    try:
        run_row(ctx, report_dir, R200, "orient_general=1", frames=2)
    finally:
        ctx.set_option("orient_general", 0)


def test_three_different_frames_in_one_batch(ctx, report_dir):
    """Three frames with their own keypoint counts under one many-level plan: the per-image lists and the per-level cell offsets
    of every image.  Each frame against its own oracle run: stage lists, counts, keypoint records, descriptors."""
    dogs, octaves, sigma, k = P18
    frames = np.stack([synth_frame(200, 150, s) for s in (3, 4, 5)])
    ctx.calculate_batch(frames, _lib.Params(dogs, octaves, sigma, k, 0))
    counts = ctx.counts().copy()
    kp, desc = (a.copy() for a in ctx.results())
    assert len(set(counts.tolist())) == 3, "the frames should differ in their keypoint counts"
    base, rep = 0, {"case": "200x150 seeds 3, 4, 5 in one batch, k 1.8", "counts": counts.tolist(), "levels": []}
    for i in range(3):
        run = row_run(R200) if i == 0 else O.OracleRun(frames[i], dogs, octaves, sigma=sigma, k=k)
        assert run.status == 0, run.error
        for stage in STAGES:
            got = ctx.stage(stage, i)
            want, wdesc = run.points(stage)
            assert got.size == want.size, f"frame {i}: {stage}: {got.size} points vs oracle {want.size}"
            for f in ("x", "y", "octave", "index"):
                assert (got[f] == want[f]).all(), f"frame {i}: {stage}: field {f}"
            assert got["scale"].tobytes() == want["scale"].tobytes(), f"frame {i}: {stage}: scale"
            if stage != "after_sort1":
                assert (got["filtered"].astype(bool) == want["filtered"].astype(bool)).all(), f"frame {i}: {stage}: filtered"
            if stage in ("after_orient", "after_sort2", "final"):
                m = ~want["filtered"].astype(bool)
                assert_bits_equal(got["orientation"][m], want["orientation"][m], f"frame {i}: {stage}: orientation")
        want, wdesc = run.points("final")
        assert counts[i] == want.size, f"frame {i}: count"
        recs = kp[base:base + want.size]
        for f in ("x", "y", "octave", "index"):
            assert (recs[f] == want[f]).all(), f"frame {i}: result field {f}"
        assert recs["scale"].tobytes() == want["scale"].tobytes() and recs["orientation"].tobytes() == want["orientation"].tobytes()
        assert (recs["has_descriptor"] == (want["n_desc"] == 128)).all()
        assert desc[base:base + want.size].tobytes() == wdesc.tobytes(), f"frame {i}: descriptors"
        got = populations(recs, dogs, octaves, sigma, k)
        assert sorted(got) == [(0, 0), (0, 2), (0, 3)] and got == populations(want, dogs, octaves, sigma, k)
        rep["levels"].append({f"({o},{j})": n for (o, j), n in sorted(got.items())})
        base += want.size
    assert base == kp.size
    with open(os.path.join(report_dir, "scale_steps.jsonl"), "a") as f:
        f.write(json.dumps(rep) + "\n")


def test_host_boundary_formats_on_a_many_level_batch(ctx):
    """8-bit frames in, sparse lists out, and the wire format's kernels (with the counting pass riding in the per-level
    descriptor launches), on two frames under the (3, 3, 1.0, 1.8) plan: tests/test_gpu_parity.py's checks of both."""
    dogs, octaves, sigma, k = P18
    params = _lib.Params(dogs, octaves, sigma, k, 0)
    frames = np.stack([synth_frame(200, 150, s) for s in (3, 4)])
    counts, kp, desc = check_u8_frames_in_sparse_lists_out(ctx, frames, params, 1000)
    want, wdesc = row_run(R200).points("final")
    assert counts[0] == want.size and desc[:want.size].tobytes() == wdesc.tobytes()
    assert len(populations(kp, dogs, octaves, sigma, k)) == 3
    kp2, desc2 = check_sparse_wire_kernels(ctx, frames, params)
    assert kp2.tobytes() == kp.tobytes() and desc2.tobytes() == desc.tobytes()


def assert_stage_lists(ctx, run, image, what):
    """The stage lists of an image, thrown or not: what the reference had formed when it stopped."""
    for stage in STAGES:
        got, want = ctx.stage(stage, image), run.points(stage)[0]
        assert got.size == want.size, f"{what}: {stage}: {got.size} points vs oracle {want.size}"
        for f in ("x", "y", "octave", "index"):
            assert (got[f] == want[f]).all(), f"{what}: {stage}: field {f}"
        assert got["scale"].tobytes() == want["scale"].tobytes(), f"{what}: {stage}: scale"


@pytest.mark.parametrize("name", sorted(K_EDGES))
def test_k_edges(ctx, report_dir, name):
    """k = 1 (every DoG scale 0), k < 1 (negative DoG scales: the nearest level is the pyramid's LAST, a level smaller than the
    keypoint's octave, and the dead 16x16 blur throws as soon as a keypoint reaches it), k = 0, k < 0 (the pyramid's own blur
    throws): status, message and counts are the oracle's."""
    w, h, seed, dogs, octaves, sigma, k, status, final, message = K_EDGES[name]
    run = edge_run(name)
    assert run.status == status and run.error.strip() == message            # (tests/test_scale_steps_host.py)
    img = synth_frame(w, h, seed)
    rc, text = ctx.calculate_batch(img[None], _lib.Params(dogs, octaves, sigma, k, 0), raise_on_error=False)
    assert (rc, text) == ((_lib.EPRECONDITION, run.error) if status else (_lib.OK, "")), (rc, text)
    assert ctx.n_images() == 1 and (ctx.status()[0] != 0) == (status != 0)
    assert ctx.counts().tolist() == [final] and ctx.total() == final
    if status == 0:
        rep = compare_run(ctx, img, dogs, octaves, False, name, report_dir, sigma=sigma, k=k, run=run)
        assert rep["final"] == final
    elif name == "k 0.9 333x257":       # thrown inside the orientation stage: the pyramid and the first lists are there
        assert_stage_lists(ctx, run, 0, name)
        assert ctx.stage("after_sort1", 0).size > 0
        for o in range(octaves):
            for j in range(dogs + 1):
                assert_bits_equal(ctx.level("gaussian", o, j, 0), run.level("gaussian", o, j), f"{name}: gaussian({o},{j})")


@pytest.mark.parametrize("order", [(9, 10), (10, 9)], ids=["thrown first", "thrown last"])
def test_k_below_one_beside_a_good_image(ctx, order):
    """k = 0.9 on two 333x257 frames in one batch: seed 9 ends in the reference's exception, seed 10 does not - its 14 keypoints
    all lie outside level (2, 3), the 84x65 level the negative scales select, and are filtered before the dead blur.  Per image:
    status, count, the stage lists; the batch's message is the thrown image's; the good image in full."""
    dogs, octaves, sigma, k = K_EDGES["k 0.9 333x257"][3:7]
    runs = {9: edge_run("k 0.9 333x257"), 10: O.OracleRun(synth_frame(333, 257, 10), dogs, octaves, sigma=sigma, k=k)}
    assert runs[9].status == 1 and runs[10].status == 0 and runs[10].points("after_sort1")[0].size > 0 and runs[10].points("final")[0].size == 0
    frames = np.stack([synth_frame(333, 257, s) for s in order])
    rc, text = ctx.calculate_batch(frames, _lib.Params(dogs, octaves, sigma, k, 0), raise_on_error=False)
    assert rc == _lib.EPRECONDITION and text == runs[9].error
    assert [int(s != 0) for s in ctx.status()] == [runs[s].status for s in order]
    assert ctx.counts().tolist() == [0, 0] and ctx.total() == 0
    for pos, s in enumerate(order):
        assert_stage_lists(ctx, runs[s], pos, f"seed {s} at {pos}")
    compare_image(ctx, runs[10], order.index(10), dogs, octaves, False, "k 0.9 good image", {})


def write_pgm(path, img):
    u8 = img.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), img)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + u8.tobytes())


def test_python_mirror_and_cli_take_k(ctx, tmp_path, monkeypatch):
    """Sift(..., k=1.8) and `python -m sift_amd.cli -k 1.8 -s 1.0`: the result file OracleRun.write_result writes."""
    from sift_amd import cli
    dogs, octaves, sigma, k = P18
    run = row_run(R200)
    run.write_result(tmp_path / "expected.txt")
    want = open(tmp_path / "expected.txt", "rb").read()
    assert len(want) > 100000
    img = row_image(R200)
    points = Sift(dogs, octaves, sigma, k, context=ctx).calculate(img)
    cli.write_result(str(tmp_path / "mirror.txt"), points)
    assert open(tmp_path / "mirror.txt", "rb").read() == want
    monkeypatch.chdir(tmp_path)
    write_pgm(tmp_path / "frame.pgm", img)
    assert cli.main(["-i", "frame.pgm", "-o", str(octaves), "-d", str(dogs), "-s", str(sigma), "-k", str(k), "-r", "1", "--no-overlay"]) == 0
    assert open(tmp_path / "interstpoints.txt", "rb").read() == want


@pytest.mark.parametrize("name", sorted(REFPIN.SCALE_CASES))
def test_hip_matches_the_reference_binary_at_other_scale_steps(ctx, name):
    """What the reference's own binary returned at (sigma, k) = (0.8, 1.5) and (1.0, 1.8) (tests/golden/refpin_scale_steps.npz): no
    oracle in between."""
    hip_against_pin(ctx, np.load(REFPIN.SCALE_PIN), REFPIN.SCALE_CASES, name)
    spec, dogs, octaves, sub, sigma, k = REFPIN.SCALE_CASES[name]
    assert len(populations(ctx.stage("final"), dogs, octaves, sigma, k)) >= 3
