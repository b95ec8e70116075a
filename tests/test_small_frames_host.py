"""Tiny and thin frames on the CPU: the rows of tests/small_frames.py are what tests/test_small_frames_gpu.py takes them for.

Every row must run to the end in the oracle with exactly the pinned candidate and final counts (literals below, re-derived
here on every run), every final keypoint with a 128-float descriptor; enough rows must end with keypoints, and enough must have a
short side of at most twice the plan's largest blur radius, that the GPU file cannot quietly degrade into ordinary frames.
The boundary table pins, per plan, the smallest width and height the oracle accepts and its exact error text one pixel below,
on each axis and on both (which check comes first).  The oracle itself is held to the reference's binary on three of the rows
by tests/test_ref_pins.py (tests/golden/refpin_small_frames.npz).
"""
import pytest

import oracle_lib as O
import small_frames as S

# row -> (candidates, final keypoints) of the oracle
COUNTS = {
    "17x300": (291, 1), "19x257": (288, 6), "30x30 2oct": (30, 4), "31x29 2oct": (29, 4), "33x47 2oct": (102, 7),
    "61x31 2oct": (121, 4), "124x31 2oct": (241, 11), "48x36 2oct": (134, 7), "47x35 2oct": (132, 5), "2000x18": (1818, 22),
    "26x26 4dogs": (58, 4), "40x40 5dogs": (215, 17), "blob 24x24": (63, 7), "blob 400x17": (962, 25), "blob 17x400": (967, 21),
    "15x15": (10, 0), "14x40": (25, 0), "15x400": (248, 0), "400x15": (287, 0), "16x1000": (900, 0), "1000x16": (801, 0),
    "65x17": (57, 0), "11x11 s1.0": (5, 0), "12x40 s1.0": (37, 0), "40x12 s1.0": (34, 0), "22x22 s2.0": (12, 0),
    "subpixel 12x12": (39, 0), "subpixel 8x200": (244, 0), "subpixel 200x8": (295, 0),
}
# the largest blur radius of each plan the rows use: (dogs, octaves, sigma, subpixel) -> radius
RADIUS_MAX = {(3, 1, 1.6, False): 10, (3, 2, 1.6, False): 14, (4, 1, 1.6, False): 14, (5, 1, 1.6, False): 19, (3, 1, 1.0, False): 6,
              (3, 1, 2.0, False): 12, (3, 1, 1.6, True): 10}

X_LONGER = "Precondition violation!\nseparableConvolveX(): kernel longer than line\n"
Y_LONGER = "Precondition violation!\nseparableConvolveY(): kernel longer than line\n"
# (sigma, dogs, octaves) -> (smallest width, smallest height, long side of the probing frames).  One pixel below, the width
# fails in separableConvolveX, the height in separableConvolveY, and with both too short the X pass throws first
# (algorithms.cpp:15-21: the row pass runs first).  The smallest side is the plan's largest radius + 1 - for two octaves twice
# that less one, the smallest size whose half (rounded up) still holds octave 1's largest kernel.
BOUNDARY = {
    (1.0, 3, 1): (7, 7, 40),
    (1.6, 3, 1): (11, 11, 40),
    (2.0, 3, 1): (13, 13, 40),
    (1.6, 4, 1): (15, 15, 40),
    (1.6, 3, 2): (29, 29, 40),
}


def test_tables_cover_each_other():
    assert sorted(COUNTS) == sorted(S.ROW) and sorted(BOUNDARY) == sorted(S.BOUNDARY_PLANS)
    assert all(r[1] in (S.synth_frame, S.blob_frame) for r in S.ROWS)


@pytest.mark.parametrize("name", S.IDS)
def test_row_runs_to_the_end_with_the_pinned_counts(name):
    run = S.row_run(name)
    assert run.status == 0, run.error
    cand, final = COUNTS[name]
    assert run.points("candidates")[0].size == cand
    pts, desc = run.points("final")
    assert pts.size == final
    assert (pts["n_desc"] == 128).all()
    dogs, octaves, sigma, subpixel = S.ROW[name][5:]
    assert max(S.plan_radii(dogs, octaves, sigma, subpixel)) == RADIUS_MAX[(dogs, octaves, sigma, subpixel)]
    if final:       # a keypoint's 16x16 window lies inside its level: in a 17-pixel side the only position is 8
        assert (pts["x"] >= 8).all() and (pts["y"] >= 8).all()
        if name in ("17x300", "blob 17x400"):
            assert set(pts["x"].tolist()) == {8}
        if name == "blob 400x17":
            assert set(pts["y"].tolist()) == {8}


def test_rows_are_not_vacuous():
    with_keypoints = [n for n in S.IDS if COUNTS[n][1] >= 1]
    assert len(with_keypoints) >= 12
    near_the_radius = [n for n in S.IDS if S.short_side(n) <= 2 * RADIUS_MAX[S.ROW[n][5:]]]
    assert len(near_the_radius) >= 10, near_the_radius
    assert any(n in with_keypoints for n in near_the_radius)
    # every row's every level is at least radius + 1 on both sides (or the oracle would have thrown) and the smallest level of the
    # table sits exactly on that edge
    assert S.short_side("30x30 2oct") // 2 == RADIUS_MAX[(3, 2, 1.6, False)] + 1


@pytest.mark.parametrize("plan", S.BOUNDARY_PLANS, ids=[f"s{p[0]} {p[1]}x{p[2]}" for p in S.BOUNDARY_PLANS])
def test_boundary(plan):
    sigma, dogs, octaves = plan
    b = S.boundary(*plan)
    assert (b["w"], b["h"], b["long"]) == BOUNDARY[plan]
    assert (b["err_w"], b["err_h"], b["err_both"]) == (X_LONGER, Y_LONGER, X_LONGER)
    w, h, long = BOUNDARY[plan]
    for size in ((w, long), (long, h), (w, h)):                 # at the edge it runs, on each axis and on both
        assert S.oracle_answer(*size, sigma, dogs, octaves) == (0, ""), size
    assert S.oracle_answer(w - 1, long, sigma, dogs, octaves) == (1, X_LONGER)
    assert S.oracle_answer(long, h - 1, sigma, dogs, octaves) == (1, Y_LONGER)
    assert S.oracle_answer(w - 1, h - 1, sigma, dogs, octaves) == (1, X_LONGER)
    radii = S.plan_radii(dogs, octaves, sigma)
    if octaves == 1:
        assert w == h == max(radii) + 1
    else:           # octave 0 alone would take max(radii of octave 0) + 1 = 11: the boundary is octave 1's
        assert S.oracle_answer(w - 1, long, sigma, dogs, 1) == (0, "") and S.oracle_answer(long, h - 1, sigma, dogs, 1) == (0, "")
        assert (w + 1) // 2 == max(radii) + 1 and w // 2 == max(radii)


def test_small_soak_skips_at_most_half():
    """tests/soak_parity.py's `small` mode against the oracle alone: of its first 300 cases (seed 1) the reference refuses at most
    half - the cap - and exactly the 138 the script's docstring states; the other modes' first cases are the ones earlier soak
    logs show."""
    import numpy as np
    import soak_parity as SP
    assert SP.SMALL_LO == 10
    rng = np.random.default_rng(1)
    refused = 0
    for _ in range(300):
        c = SP.draw_small(rng)
        assert SP.SMALL_LO <= min(c["w"], c["h"]) <= 64 and max(c["w"], c["h"]) <= 2000 and c["octaves"] in (1, 2) and 1 <= c["frames"] <= 3
        refused += O.OracleRun(SP.case_image(c), c["dogs"], c["octaves"], sigma=c["sigma"], k=c["k"], subpixel=c["subpixel"]).status != 0
    assert refused == 138 and refused <= 150
    rng = np.random.default_rng(7)      # profiles/soak_parity_scale_steps.txt: the first cases of `soak_parity.py 270 7`
    first = [SP.draw(rng) for _ in range(3)]
    assert [(c["w"], c["h"], c["octaves"], c["sigma"], c["k"], c["frames"], c["seed"]) for c in first] == \
        [(424, 398, 2, 1.6, 1.7, 3, 137826), (517, 163, 2, 1.2, 1.5, 2, 734291), (1292, 631, 1, 1.6, 1.5, 2, 863463)]
    c = SP.draw_big(np.random.default_rng(1))
    assert (c["w"], c["h"], c["dogs"], c["octaves"], c["seed"], c["k"]) == (2465, 1468, 3, 5, 261335, O.K_SQRT2)


def test_issue_examples():
    """9x9 throws in the X pass, 14x40 runs (sigma 1.6, 3 DoGs, 1 octave)."""
    assert S.oracle_answer(9, 9, 1.6, 3, 1) == (1, X_LONGER)
    assert S.oracle_answer(14, 40, 1.6, 3, 1) == (0, "")
    assert 10 <= BOUNDARY[(1.6, 3, 1)][0] <= 14
