"""Tiny and thin frames: the inputs of tests/test_small_frames_host.py and tests/test_small_frames_gpu.py (a helper, no tests).

The reference's only size condition is vigra's `w >= radius + 1` and `h >= radius + 1` per blur (separableConvolveX / Y), so it
runs frames whose sides are barely longer than its largest blur radius: both halos of every blur tile or strip leave the image
at once, a reflected halo spans the whole line, the extremum scan sees images smaller than one of its tiles, and the 16x16
descriptor window of a keypoint in a 17-pixel-wide level touches both borders.  ROWS are such frames; both test files import
the table, so the GPU rows are exactly the rows whose oracle populations the host file pins.

The boundary search asks the ORACLE alone for the smallest side it accepts under a plan - never the library.
"""
import functools

import oracle_lib as O
import scale_ref
from sift_amd.synthetic import blob_frame, synth_frame

# (name, generator, w, h, seed, dogs, octaves, sigma, subpixel); k = sqrt(2) throughout
ROWS = [
    # rows that end with keypoints and descriptors
    ("17x300", synth_frame, 17, 300, 1, 3, 1, 1.6, False),              # the only legal keypoint column is x = 8
    ("19x257", synth_frame, 19, 257, 1, 3, 1, 1.6, False),
    ("30x30 2oct", synth_frame, 30, 30, 1, 3, 2, 1.6, False),           # octave 1 is 15x15
    ("31x29 2oct", synth_frame, 31, 29, 1, 3, 2, 1.6, False),           # odd sizes: 16x15
    ("33x47 2oct", synth_frame, 33, 47, 1, 3, 2, 1.6, False),
    ("61x31 2oct", synth_frame, 61, 31, 1, 3, 2, 1.6, False),
    ("124x31 2oct", synth_frame, 124, 31, 1, 3, 2, 1.6, False),         # two scan tiles wide, rows 16-byte aligned in octave 0 only
    ("48x36 2oct", synth_frame, 48, 36, 1, 3, 2, 1.6, False),           # both octaves 16-byte aligned: the streaming and kept-pixels forms fit
    ("47x35 2oct", synth_frame, 47, 35, 1, 3, 2, 1.6, False),
    ("2000x18", synth_frame, 2000, 18, 1, 3, 1, 1.6, False),            # a strip: many tiles wide, lower than any radius doubled
    ("26x26 4dogs", synth_frame, 26, 26, 1, 4, 1, 1.6, False),
    ("40x40 5dogs", synth_frame, 40, 40, 1, 5, 1, 1.6, False),
    ("blob 24x24", blob_frame, 24, 24, 3, 3, 1, 1.6, False),
    ("blob 400x17", blob_frame, 400, 17, 3, 3, 1, 1.6, False),          # the only legal keypoint row is y = 8
    ("blob 17x400", blob_frame, 17, 400, 3, 3, 1, 1.6, False),
    # rows that run to the end with candidates but no final keypoint: pyramid, scan, edge filter, cleanup, an empty descriptor stage
    ("15x15", synth_frame, 15, 15, 1, 3, 1, 1.6, False),
    ("14x40", synth_frame, 14, 40, 1, 3, 1, 1.6, False),
    ("15x400", synth_frame, 15, 400, 1, 3, 1, 1.6, False),
    ("400x15", synth_frame, 400, 15, 1, 3, 1, 1.6, False),
    ("16x1000", synth_frame, 16, 1000, 1, 3, 1, 1.6, False),            # 16-byte aligned rows of four lane vectors
    ("1000x16", synth_frame, 1000, 16, 1, 3, 1, 1.6, False),
    ("65x17", synth_frame, 65, 17, 1, 3, 1, 1.6, False),                # one column into the second scan tile
    ("11x11 s1.0", synth_frame, 11, 11, 1, 3, 1, 1.0, False),
    ("12x40 s1.0", synth_frame, 12, 40, 1, 3, 1, 1.0, False),
    ("40x12 s1.0", synth_frame, 40, 12, 1, 3, 1, 1.0, False),
    ("22x22 s2.0", synth_frame, 22, 22, 1, 3, 1, 2.0, False),
    ("subpixel 12x12", synth_frame, 12, 12, 1, 3, 1, 1.6, True),        # the doubled input is 24x24
    ("subpixel 8x200", synth_frame, 8, 200, 1, 3, 1, 1.6, True),        # ... 16x400
    ("subpixel 200x8", synth_frame, 200, 8, 1, 3, 1, 1.6, True),
]
ROW = {r[0]: r for r in ROWS}
assert len(ROW) == len(ROWS)
IDS = [r[0] for r in ROWS]


def row_image(name):
    gen, w, h, seed = ROW[name][1:5]
    return gen(w, h, seed)


@functools.lru_cache(maxsize=None)
def row_run(name):
    """The oracle's run of a row, shared by every test of the session (nothing may change it)."""
    dogs, octaves, sigma, subpixel = ROW[name][5:]
    return O.OracleRun(row_image(name), dogs, octaves, sigma=sigma, subpixel=subpixel)


def plan_radii(dogs, octaves, sigma, subpixel=False, k=O.K_SQRT2):
    """The radius of every blur the pyramid of a plan runs (sift.cpp:386-411 by tests/scale_ref.py, radii from the oracle's taps):
    the doubling blur (sigma 1.0) with subpixel, g(0,0) = blur(image, sigma), then every level (o, j >= 1) with its own scale -
    the decimating blur between octaves repeats the scale of level (o, dogs - 1)."""
    gauss = scale_ref.schedule(dogs, octaves, sigma, k)[0]
    sigmas = ([1.0] if subpixel else []) + [float(sigma)] + [float(gauss[o][j]) for o in range(octaves) for j in range(1, dogs + 1)]
    return [O.gauss_taps(s)[0] for s in sigmas]


def short_side(name):
    """The short side of the image the pyramid is built on (the doubled one with subpixel)."""
    w, h = ROW[name][2:4]
    return min(w, h) * (2 if ROW[name][8] else 1)


# ---- the size boundary: the smallest side the oracle accepts under a plan ----------------------------------------------------
BOUNDARY_PLANS = [(1.0, 3, 1), (1.6, 3, 1), (2.0, 3, 1), (1.6, 4, 1), (1.6, 3, 2)]      # (sigma, dogs, octaves)
BOUNDARY_SEED = 1


def boundary_frame(w, h):
    return synth_frame(w, h, BOUNDARY_SEED)


def oracle_answer(w, h, sigma, dogs, octaves):
    """-> (status, error text) of the oracle for the boundary frame of that size."""
    run = O.OracleRun(boundary_frame(w, h), dogs, octaves, sigma=sigma)
    return run.status, run.error


@functools.lru_cache(maxsize=None)
def boundary(sigma, dogs, octaves):
    """-> dict: `long`, the long side of the probing frames (40, doubled until the oracle accepts long x long: 40 is too short
    for some plans); `w`, `h`: the smallest width s for which the oracle accepts s x long, the smallest height for long x s (walked
    down from `long` to the first refusal; with two octaves that is the size at which octave 1 first fails while octave 0
    passes); `err_w`, `err_h`, `err_both`: its error text for (w - 1) x long, long x (h - 1), (w - 1) x (h - 1)."""
    long = 40
    while oracle_answer(long, long, sigma, dogs, octaves)[0] != 0:
        long *= 2
        assert long <= 640, "no frame of this plan runs"
    out = {"long": long}
    for axis in ("w", "h"):
        s = long
        while s > 1:
            size = (s - 1, long) if axis == "w" else (long, s - 1)
            status, err = oracle_answer(*size, sigma, dogs, octaves)
            if status != 0:
                out["err_" + axis] = err
                break
            s -= 1
        assert s > 1, "the oracle refused no size"
        out[axis] = s
    status, out["err_both"] = oracle_answer(out["w"] - 1, out["h"] - 1, sigma, dogs, octaves)
    assert status != 0
    return out
