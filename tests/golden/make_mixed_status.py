#!/usr/bin/env python3
"""Generates tests/golden/mixed_status_frames.npz: seven 256 x 192 frames of which some end in the reference's exception of
the dead 16x16 blur (App. B-14, sift.cpp:184) and some do not, for the batches of tests/test_mixed_status_gpu.py, with the
oracle's verdict for each (tests/test_mixed_status_host.py runs the oracle on the stored frames and asserts them).

  frames      uint8 [7, 192, 256]: twelve isolated Gaussian blobs on a flat background, rounded to 8 bits (storing them
              removes any dependence on a platform's exp); F5 is a constant frame
  status      int32 [7]: the oracle's status (0, or 1: the reference throws)
  error       the oracle's error text per frame ("" where it does not throw)
  counts      int64 [7, 5]: points after candidates, after_sort1, after_orient, after_sort2, final (where it throws, the
              lists it had formed by then: the last three are empty)
  params      dogsPerEpoch, octaves, sigma, k, subpixel

With 5 DoGs per octave and 2 octaves, blobs of sigma <= 4 give keypoints at DoG indices 1 .. 3 of octave 0 and 1 .. 2 of
octave 1 and never one in the level whose dead blur would violate Vigra's precondition; blobs of sigma >= 6 always give one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

W, H = 256, 192
DOGS, OCTAVES, SIGMA, SUBPIXEL = 5, 2, 1.6, 0
STAGES = ("candidates", "after_sort1", "after_orient", "after_sort2", "final")
# (blob sigma, seed); None: the constant frame
FRAMES = [(2.0, 1), (6.0, 1), (3.0, 2), (10.0, 2), (1.5, 3), None, (4.0, 1)]
THROWN = (1, 3)


def blobs(w, h, sig, seed, n=12, amp=80.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 100.0)
    for _ in range(n):
        cx, cy = rng.uniform(30, w - 30), rng.uniform(30, h - 30)
        img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sig * sig))
    return np.round(np.clip(img, 0, 255)).astype(np.float32)


def main():
    frames = np.stack([np.full((H, W), 100.0, np.float32) if f is None else blobs(W, H, *f) for f in FRAMES])
    u8 = frames.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), frames)
    status, errors, counts = [], [], []
    for i, img in enumerate(u8):
        run = O.OracleRun(img.astype(np.float32), DOGS, OCTAVES, sigma=SIGMA)
        status.append(run.status)
        errors.append(run.error)
        counts.append([run.points(s)[0].size for s in STAGES])
        print(f"F{i}: {FRAMES[i]}: status {run.status} {run.error!r} counts {counts[-1]}")
        run.close()
    assert [i for i, s in enumerate(status) if s] == list(THROWN), status
    np.savez_compressed(os.path.join(HERE, "mixed_status_frames.npz"), frames=u8, status=np.array(status, np.int32),
                        error=np.array(errors), counts=np.array(counts, np.int64),
                        params=np.array([DOGS, OCTAVES, SIGMA, O.K_SQRT2, SUBPIXEL], np.float64))


if __name__ == "__main__":
    main()
