"""The frames of tests/golden/mixed_status_frames.npz (make_mixed_status.py) behave on the CPU oracle as the file says: the
condition under which tests/test_mixed_status_gpu.py means anything.  Every "good" image of its batches really has keypoints,
the constant one really has none without throwing, and every "thrown" one really ends in the reference's exception of the
dead 16x16 blur (App. B-14, sift.cpp:184).  Runs the oracle only."""
import os

import numpy as np
import pytest

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixed_status_frames.npz")
STAGES = ("candidates", "after_sort1", "after_orient", "after_sort2", "final")
GOOD, THROWN, CONSTANT = (0, 2, 4, 6), (1, 3), 5


def load_fixture():
    g = np.load(GOLDEN)
    dogs, octaves, sigma, k, subpixel = g["params"].tolist()
    return g, (int(dogs), int(octaves), float(sigma), float(k), int(subpixel))


def oracle_runs(g, params):
    dogs, octaves, sigma, k, subpixel = params
    return [O.OracleRun(f.astype(np.float32), dogs, octaves, sigma=sigma, k=k, subpixel=bool(subpixel)) for f in g["frames"]]


@pytest.fixture(scope="module")
def fixture_and_runs():
    g, params = load_fixture()
    return g, params, oracle_runs(g, params)


def test_fixture_layout(fixture_and_runs):
    g, params, _ = fixture_and_runs
    assert g["frames"].dtype == np.uint8 and g["frames"].shape == (7, 192, 256)
    assert params == (5, 2, 1.6, O.K_SQRT2, 0)
    assert g["status"].shape == (7,) and g["error"].shape == (7,) and g["counts"].shape == (7, 5)
    assert (g["frames"][CONSTANT] == 100).all()
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_oracle_gives_the_stored_verdicts(fixture_and_runs):
    g, _, runs = fixture_and_runs
    for i, run in enumerate(runs):
        counts = [run.points(s)[0].size for s in STAGES]
        print(f"F{i}: status {run.status} {run.error!r} counts {counts}")
        assert run.status == int(g["status"][i]), i
        assert run.error == str(g["error"][i]), i
        assert counts == g["counts"][i].tolist(), i
        if i in THROWN:
            assert run.status == 1 and run.error != "" and "separableConvolveX(): kernel longer than line" in run.error, i
            assert counts[1] > 0 and counts[2:] == [0, 0, 0], i      # it throws inside the orientation assignment
            continue
        assert run.status == 0 and run.error == "", i
        if i == CONSTANT:
            assert counts[4] == 0 and counts[0] > 0, i          # every interior pixel ties, every candidate is filtered
        else:
            assert i in GOOD and 50 < counts[4] <= 255, i
    assert g["counts"][list(THROWN), 4].sum() == 0
