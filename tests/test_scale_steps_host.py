"""Scale steps other than sqrt(2), on the CPU: the inputs of tests/test_scale_steps_gpu.py are what that file takes them for.

`k` decides which Gaussian level a keypoint takes its gradient maps, its orientation histogram and its descriptor from
(Sift::_findNearestGaussian, sift.cpp:205-218, over the whole pyramid).  At k = sqrt(2) every scanned DoG scale is below 1.9 and
that level is (0, 0) for every keypoint; the rows of ROWS select two to four levels.  This file checks tests/scale_ref.py (the
schedule and the search restated from the reference's source) against the oracle's own scales, and recomputes for every row
what the GPU tests rely on: the oracle ends with the listed status, and each listed level gets exactly the listed number of the
oracle's final keypoints.  While it passes, the GPU tests cannot quietly degrade into single-level runs.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import scale_ref
from sift_amd.synthetic import blob_frame, synth_frame

# id -> (frame generator, w, h, seed, dogs, octaves, sigma, k, subpixel, final keypoints, {gradient level: final keypoints})
ROWS = {
    "160x120 5x2 s0.8 k1.5": (synth_frame, 160, 120, 1, 5, 2, 0.8, 1.5, False, 762, {(0, 0): 635, (0, 2): 39, (0, 3): 34, (0, 4): 54}),   # four levels at the smallest frame
    "160x120 3x2 s1.6 k2.0": (synth_frame, 160, 120, 1, 3, 2, 1.6, 2.0, False, 324, {(0, 0): 257, (0, 2): 67}),   # largest sigma 12.8: radius 38, beyond the fused blur
    "160x120 3x2 s1.0 k2.2": (synth_frame, 160, 120, 1, 3, 2, 1.0, 2.2, False, 514, {(0, 0): 443, (0, 2): 71}),
    "200x150 3x3 s1.0 k1.8": (synth_frame, 200, 150, 3, 3, 3, 1.0, 1.8, False, 754, {(0, 0): 617, (0, 2): 107, (0, 3): 30}),   # (0,3) is octave 0's TOP level
    "240x180 4x3 s0.8 k1.5": (synth_frame, 240, 180, 2, 4, 3, 0.8, 1.5, False, 1463, {(0, 0): 1277, (0, 2): 107, (0, 3): 25, (0, 4): 54}),   # (0,4) is the top level
    "322x250 3x4 s1.0 k1.6": (synth_frame, 322, 250, 12, 3, 4, 1.0, 1.6, False, 1988, {(0, 0): 1955, (0, 2): 30, (0, 3): 3}),   # width 2 mod 4, a level with 3 keypoints
    "333x257 3x3 s1.6 k1.7": (synth_frame, 333, 257, 9, 3, 3, 1.6, 1.7, False, 1485, {(0, 0): 1380, (0, 2): 105}),   # odd sizes, the default sigma
    "blobs 352x264 3x3 s1.0 k1.8": (blob_frame, 352, 264, 5, 3, 3, 1.0, 1.8, False, 455, {(0, 0): 336, (0, 2): 107, (0, 3): 12}),   # dense lattice
    "blobs 352x264 4x3 s0.8 k1.5": (blob_frame, 352, 264, 5, 4, 3, 0.8, 1.5, False, 1029, {(0, 0): 901, (0, 2): 118, (0, 3): 9, (0, 4): 1}),   # a level with one keypoint
    "200x150 subpixel 3x2 s1.0 k1.8": (synth_frame, 200, 150, 3, 3, 2, 1.0, 1.8, True, 358, {(0, 2): 342, (0, 0): 16}),   # most keypoints away from level 0
    "642x481 3x2 s0.5 k3.0": (synth_frame, 642, 481, 7, 3, 2, 0.5, 3.0, False, 8211, {(0, 0): 6792, (0, 2): 1419}),   # the two nearest Gaussians tie in real arithmetic
}

STD_DEV = "Precondition violation!\nKernel1D::initGaussian(): Standard deviation must be >= 0."
# the edges of k itself.  id -> (w, h, seed, dogs, octaves, sigma, k, status, final keypoints, message)
K_EDGES = {
    "k 1.0 333x257": (333, 257, 9, 3, 3, 1.6, 1.0, 0, 4, ""),          # every level has sigma 1.6, every DoG scale is 0
    "k 0.9 333x257": (333, 257, 9, 3, 3, 1.6, 0.9, 1, 0, STD_DEV),     # a negative DoG scale reaches the dead 16x16 blur (sift.cpp:184)
    "k 0.9 200x150": (200, 150, 3, 3, 3, 1.6, 0.9, 0, 0, ""),          # ... and does not where no keypoint reaches it
    "k 0.0 200x150": (200, 150, 3, 3, 2, 1.6, 0.0, 0, 0, ""),
    "k -1.5 200x150": (200, 150, 3, 3, 2, 1.6, -1.5, 1, 0, STD_DEV),   # thrown by the pyramid's own blur
}


def row_image(name):
    gen, w, h, seed = ROWS[name][:4]
    return gen(w, h, seed)


@functools.lru_cache(maxsize=None)
def row_run(name):
    """The oracle's run of a row, shared by every test of the session (nothing may change it)."""
    dogs, octaves, sigma, k, subpixel = ROWS[name][4:9]
    return O.OracleRun(row_image(name), dogs, octaves, sigma=sigma, k=k, subpixel=subpixel)


@functools.lru_cache(maxsize=None)
def edge_run(name):
    w, h, seed, dogs, octaves, sigma, k = K_EDGES[name][:7]
    return O.OracleRun(synth_frame(w, h, seed), dogs, octaves, sigma=sigma, k=k)


def populations(points, dogs, octaves, sigma, k):
    """{gradient level: how many of `points` select it}, by tests/scale_ref.py."""
    return scale_ref.level_populations(points, scale_ref.schedule(dogs, octaves, sigma, k)[2])


def assert_schedule_is_the_oracles(run, dogs, octaves, sigma, k, what):
    gauss, dog, nearest = scale_ref.schedule(dogs, octaves, sigma, k)
    for o in range(octaves):
        for j in range(dogs + 1):
            assert np.float32(run.scale("gaussian", o, j)).tobytes() == gauss[o][j].tobytes(), f"{what}: gaussian({o},{j}) scale"
        for j in range(dogs):
            assert np.float32(run.scale("dog", o, j)).tobytes() == dog[o][j].tobytes(), f"{what}: dog({o},{j}) scale"


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_is_a_many_level_run(name):
    dogs, octaves, sigma, k, subpixel, final, levels = ROWS[name][4:]
    run = row_run(name)
    assert run.status == 0, run.error
    assert_schedule_is_the_oracles(run, dogs, octaves, sigma, k, name)
    pts, desc = run.points("final")
    assert pts.size == final
    assert (pts["n_desc"] == 128).all()                      # every keypoint has a descriptor
    got = populations(pts, dogs, octaves, sigma, k)
    assert got == levels and len(levels) >= 2 and min(levels.values()) >= 1
    # the oracle formed gradient maps for exactly these levels (it forms a level's when a keypoint first selects it)
    have = {(o, j) for o in range(octaves) for j in range(dogs + 1) if run.level("magnitude", o, j) is not None}
    assert have == set(levels)


def test_sqrt2_selects_level_zero_only():
    """What makes the rows above necessary: at k = sqrt(2) every scanned DoG level of the suite's fixed cases selects (0, 0)."""
    for dogs, octaves in [(3, 1), (3, 2), (3, 3), (3, 4), (4, 2)]:
        nearest = scale_ref.schedule(dogs, octaves, 1.6, O.K_SQRT2)[2]
        assert {nearest[o][i] for o in range(octaves) for i in range(1, dogs - 1)} == {(0, 0)}, (dogs, octaves)


def test_k3_tie_is_decided_by_float_rounding():
    """sigma 0.5, k 3: the Gaussian scales are 0.5, 0.5, 1.5, 4.5 and DoG (0, 1) has scale 1.0 - as far from 0.5 as from 1.5 in
    real arithmetic.  Every operand is a float here and the differences are exact, so the strict `<` keeps the FIRST: (0, 0);
    DoG (1, 1) = 3.0 lies between 1.5 and 4.5 and takes the first of those, (0, 2)."""
    gauss, dog, nearest = scale_ref.schedule(3, 2, 0.5, 3.0)
    assert [float(g) for g in gauss[0]] == [0.5, 0.5, 1.5, 4.5] and float(dog[0][1]) == 1.0 and float(dog[1][1]) == 3.0
    assert nearest[0][1] == (0, 0) and nearest[1][1] == (0, 2)


@pytest.mark.parametrize("name", sorted(K_EDGES))
def test_k_edge_ends_as_listed(name):
    w, h, seed, dogs, octaves, sigma, k, status, final, message = K_EDGES[name]
    run = edge_run(name)
    assert run.status == status, run.error
    assert run.error.strip() == message
    assert run.points("final")[0].size == final
    if status == 0 or name == "k 0.9 333x257":      # (k = -1.5 throws while the pyramid is built: no schedule to read)
        assert_schedule_is_the_oracles(run, dogs, octaves, sigma, k, name)


def test_negative_dog_scale_selects_a_level_smaller_than_the_octave():
    """k = 0.9: every scanned DoG scale is negative, |gaussian - scale| is smallest for the pyramid's smallest sigma, which is the LAST
    level, (2, 3) - a level of octave 2 for keypoints of octaves 0 and 1."""
    gauss, dog, nearest = scale_ref.schedule(3, 3, 1.6, 0.9)
    assert all(float(row[0]) == 0 and float(row[1]) < 0 and float(row[2]) < 0 for row in dog)
    assert {nearest[o][1] for o in range(3)} == {(2, 3)}
