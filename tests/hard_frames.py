"""Seeded frames of the kinds the suite's usual content (sift_amd.synthetic: value noise, blob lattice; the parrot) is not:
negative pixels, two-valued, saturated plateaus, exact mirror symmetry, periodic patterns, isolated impulses, other value
ranges.  `sift_hip_calculate_batch` takes any float image, and these reach code the usual content never does:

    signed      zero-mean pixels.  The orientation histogram weights each sample with the blurred level's raw pixel value
                 and every sample lands in bin 0 (B-9): bin 0 goes negative, the 35 empty bins are the
                maxima, `_findPeaks` returns several peaks (B-18) and the keypoint is duplicated per peak.
    binary      h0 = 0 in places: NaN orientations (B-9), which the descriptor stage then adds into the orientation map in
                place (B-11), and all-zero descriptors.
    saturated   plateaus of exactly 0 and 255: DoG exactly 0 over regions, ties in the extrema scan.
    mirror4     four mirrored copies of one quadrant: exact ties between mirrored extrema and gradients.
    checker, stripes, impulses   thousands of candidates from ties, (nearly) all filtered.
    unit, u16range               the same content scaled to 0..1 (nothing passes the contrast test) and to 0..65535.

In the style of sift_amd/synthetic.py: integer arithmetic before the final cast (one correctly rounded float32 division for
`unit`), bit-reproducible anywhere.  tests/test_hard_frames_host.py asserts, on the CPU oracle, the property that makes each
frame hard, so that the GPU tests built on them cannot go vacuous.
"""
from __future__ import annotations

import numpy as np

from sift_amd.synthetic import _splitmix64, synth_frame

CELL = 12          # checker cell, stripe period
N_IMPULSES = 60


def _int_frame(width, height, seed):
    return synth_frame(width, height, seed).astype(np.int32)


def _f32(a):
    return np.ascontiguousarray(a.astype(np.float32))


def signed(width, height, seed):
    return _f32(_int_frame(width, height, seed) - 128)


def binary(width, height, seed):
    return _f32(255 * (_int_frame(width, height, seed) > 128).astype(np.int32))


def saturated(width, height, seed):
    return _f32(np.clip((_int_frame(width, height, seed) - 110) * 6, 0, 255))


def mirror4(width, height, seed):
    assert width % 2 == 0 and height % 2 == 0
    q = _int_frame(width // 2, height // 2, seed)
    return _f32(np.block([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]]))


def checker(width, height, seed=0):
    ys, xs = np.meshgrid(np.arange(height, dtype=np.int32), np.arange(width, dtype=np.int32), indexing="ij")
    return _f32(255 * (((xs + seed) // CELL + (ys + seed) // CELL) & 1))


def stripes(width, height, seed=0):
    ys = np.arange(height, dtype=np.int32)
    row = 255 * ((((ys + seed) % CELL) * 2) // CELL)       # CELL / 2 rows of 0, CELL / 2 rows of 255
    return _f32(np.repeat(row[:, None], width, axis=1))


def impulses(width, height, seed):
    """About N_IMPULSES single pixels of 255 on 0 (two draws may coincide), at least 2 px inside the border."""
    with np.errstate(over="ignore"):
        key = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1A9015E5) * np.uint64(0xD1B54A32D192ED03) \
            + np.arange(N_IMPULSES, dtype=np.uint64)
    r = _splitmix64(key)
    xs = 2 + ((r >> np.uint64(40)) % np.uint64(width - 4)).astype(np.int64)
    ys = 2 + ((r >> np.uint64(8)) % np.uint64(height - 4)).astype(np.int64)
    out = np.zeros((height, width), np.int32)
    out[ys, xs] = 255
    return _f32(out)


def unit(width, height, seed):
    return np.ascontiguousarray(synth_frame(width, height, seed) / np.float32(255))


def u16range(width, height, seed):
    return _f32(_int_frame(width, height, seed) * 257)


GENERATORS = {"signed": signed, "binary": binary, "saturated": saturated, "mirror4": mirror4, "checker": checker,
              "stripes": stripes, "impulses": impulses, "unit": unit, "u16range": u16range}

SEED = 3
# mirror4: the quadrant is synth_frame(w / 2, h / 2, 4).  impulses: a seed at which the frame keeps at least 20 keypoints at
# both sizes without subpixel too (most seeds leave 11 .. 19 at 192x144; tests/test_hard_frames_host.py holds the condition)
SEEDS = {"mirror4": 4, "impulses": 22}


def hard_frame(kind, width, height, seed=None):
    img = GENERATORS[kind](width, height, SEEDS.get(kind, SEED) if seed is None else seed)
    assert img.dtype == np.float32 and img.shape == (height, width) and img.flags.c_contiguous
    return img


# (kind, width, height, dogs, octaves, subpixel): 160x120 with 3 DoGs x 2 octaves, 192x144 with 3 DoGs x 3 octaves with and
# without subpixel
SIZES = [(160, 120, 3, 2, False), (192, 144, 3, 3, False), (192, 144, 3, 3, True)]
CASES = [(kind,) + size for kind in GENERATORS for size in SIZES]


def case_id(case):
    kind, w, h, dogs, octaves, sub = case
    return f"{kind} {w}x{h} {dogs}x{octaves}" + (" subpixel" if sub else "")
