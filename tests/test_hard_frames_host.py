"""The frames of tests/hard_frames.py through the CPU oracle: per frame, the property that makes it hard.  These are
conditions, not measurements - they keep tests/test_hard_frames_gpu.py from going vacuous (a `signed` frame whose keypoints all
have one peak would not run the fallback it is there for).  The oracle itself stands on the reference's binary for the four
frames of tests/golden/make_ref_pins.py:HARD_CASES (tests/test_ref_pins.py)."""
import numpy as np
import pytest

import oracle_lib as O
from hard_frames import CASES, SIZES, case_id, hard_frame


def run_case(kind, w, h, dogs, octaves, sub):
    run = O.OracleRun(hard_frame(kind, w, h), dogs, octaves, subpixel=sub)
    assert run.status == 0, run.error
    return run


def key(p):
    return (int(p["x"]), int(p["y"]), int(p["octave"]), int(p["index"]))


def test_generators_are_reproducible_and_what_their_names_say():
    from sift_amd.synthetic import synth_frame
    s = synth_frame(160, 120, 3)
    assert np.array_equal(hard_frame("signed", 160, 120), s - 128) and hard_frame("signed", 160, 120).min() < 0
    b = hard_frame("binary", 160, 120)
    assert set(np.unique(b).tolist()) == {0.0, 255.0} and np.array_equal(b == 255, s > 128)
    sat = hard_frame("saturated", 160, 120)
    assert np.array_equal(sat, np.clip((s - 110) * 6, 0, 255)) and (sat == 0).sum() > 500 and (sat == 255).sum() > 500
    m = hard_frame("mirror4", 160, 120)
    assert np.array_equal(m, m[:, ::-1]) and np.array_equal(m, m[::-1]) and np.array_equal(m[:60, :80], synth_frame(80, 60, 4))
    c = hard_frame("checker", 160, 120)
    assert set(np.unique(c).tolist()) == {0.0, 255.0} and np.array_equal(c[12:, 12:], c[:-12, :-12]) and np.array_equal(c[12:], 255 - c[:-12])
    st = hard_frame("stripes", 192, 144)
    assert (st == st[:, :1]).all() and np.array_equal(st[12:], st[:-12]) and np.array_equal(st[6:], 255 - st[:-6])
    imp = hard_frame("impulses", 192, 144)
    assert set(np.unique(imp).tolist()) == {0.0, 255.0} and 50 <= int((imp == 255).sum()) <= 60
    u = hard_frame("unit", 160, 120)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() <= 1 and np.array_equal(u, s / np.float32(255))
    assert np.array_equal(hard_frame("u16range", 160, 120), s * 257) and hard_frame("u16range", 160, 120).max() > 40000
    for case in CASES:
        assert hard_frame(*case[:3]).tobytes() == hard_frame(*case[:3]).tobytes()


def test_signed_frame_gives_keypoints_several_orientation_peaks():
    """Zero-mean pixels: the 36-bin histogram's only filled bin goes negative, the empty bins are the maxima and `_findPeaks`
    returns a set of several (sift.cpp:220-286).  sift.cpp:190-199 then appends one record per peak - the first peak again,
    App. B-18 - behind the list, while the point itself keeps the smallest peak."""
    run = run_case("signed", 160, 120, 3, 2, False)
    s1, _ = run.points("after_sort1")
    ao, _ = run.points("after_orient")
    assert ao.size > s1.size
    head, extra = ao[:s1.size], ao[s1.size:]
    assert [key(p) for p in head] == [key(p) for p in s1]
    assert len({key(p) for p in s1}) == s1.size
    groups = {}
    for p in extra:                       # the records of one keypoint are appended together, peaks ascending (std::set)
        groups.setdefault(key(p), []).append(float(p["orientation"]))
    assert len(groups) >= 50, f"only {len(groups)} survivors with more than one peak"
    by_key = {key(p): p for p in head}
    assert sum(len(v) for v in groups.values()) == extra.size
    for k, peaks in groups.items():
        p = by_key[k]
        assert not p["filtered"] and not np.isnan(peaks).any()
        assert len(peaks) > 1 and peaks == sorted(set(peaks)), (k, peaks)      # after_orient holds the point + one record per peak
        own = float(p["orientation"])
        assert own == min(peaks)                                               # its own orientation: the smallest peak ...
        assert ([own] + peaks).count(own) == 2                                 # ... which occurs twice (B-18)
    for p in head:                                                             # single-peak and border points: no record appended
        if key(p) not in groups:
            assert sum(1 for q in ao if key(q) == key(p)) == 1
    fin, fdesc = run.points("final")
    assert fin.size >= 20 and len({key(p) for p in fin}) < fin.size            # records that share coordinates reach the descriptor stage


@pytest.mark.parametrize("size", SIZES, ids=[f"{s[0]}x{s[1]}" + (" subpixel" if s[4] else "") for s in SIZES])
def test_binary_frame_gives_nan_orientations_and_zero_descriptors(size):
    """h0 = 0 (App. B-9): the parabola through (355, 0), (5, 0), (15, 0) has no vertex; the NaN is added into the orientation
    map in place (B-11, sift.cpp:80-92) for every later keypoint whose window overlaps."""
    run = run_case("binary", *size)
    fin, fdesc = run.points("final")
    assert int(np.isnan(fin["orientation"]).sum()) >= 1
    valid = fin["n_desc"] == 128
    assert int((valid & (fdesc == 0).all(axis=1)).sum()) >= 1
    assert fin.size >= 20


@pytest.mark.parametrize("kind", ["stripes", "unit"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{s[0]}x{s[1]}" + (" subpixel" if s[4] else "") for s in SIZES])
def test_frames_whose_candidates_are_all_filtered(kind, size):
    run = run_case(kind, *size)
    cand, _ = run.points("candidates")
    assert cand.size > 1000 and cand["filtered"].all()
    for stage in ("after_sort1", "after_orient", "after_sort2", "final"):
        assert run.points(stage)[0].size == 0


def test_impulses_with_subpixel_give_tens_of_thousands_of_candidates():
    run = run_case("impulses", 192, 144, 3, 3, True)
    assert run.points("candidates")[0].size > 50000
    assert run.points("final")[0].size >= 20


OTHER = [c for c in CASES if c[0] not in ("stripes", "unit")]


@pytest.mark.parametrize("case", OTHER, ids=[case_id(c) for c in OTHER])
def test_every_other_frame_keeps_keypoints(case):
    run = run_case(*case)
    assert run.points("final")[0].size >= 20


def test_saturated_and_mirrored_frames_have_their_ties():
    """Plateaus of exactly 0 / 255: DoG levels exactly flat over regions.  The mirrored frame: the blur sums its taps in one
    fixed order, which the mirror image meets reversed, so mirrored DoG samples agree to a few ulp of 128 (2^-16 each, far
    below any difference between unrelated pixels) but not all to the bit: twin extrema that tie or nearly tie."""
    run = run_case("saturated", 160, 120, 3, 2, False)
    assert int((run.level("dog", 0, 0) == 128).sum()) > 200        # a DoG level is stored as 128 + difference
    run = run_case("mirror4", 160, 120, 3, 2, False)
    d = run.level("dog", 0, 1)
    for m in (d[:, ::-1], d[::-1]):
        assert float(np.abs(d - m).max()) <= 16 * 2.0 ** -16 and int((d == m).sum()) > 1000


def test_signed_views_hold_records_that_share_coordinates():
    """What tests/test_hard_frames_gpu.py's matching case rests on: two views of one `signed` frame 8 columns apart end with
    status 0, their final lists hold several records per location, and the match lists (host checker) hold equal coordinate
    rows - samples a RANSAC draw can take twice."""
    import match_ref as M
    from hard_frames import signed
    big = signed(272, 192, 1)
    fin = []
    for img in (np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])):
        run = O.OracleRun(img, 3, 3)
        assert run.status == 0, run.error
        k, d = run.points("final")
        assert len({key(p) for p in k}) < k.size - 50
        fin.append((k, d))
    (ka, da), (kb, db) = fin
    va, vb = ka["n_desc"] == 128, kb["n_desc"] == 128
    fwd, rev = M.knn2(da, db, va, vb), M.knn2(db, da, vb, va)
    for cross in (False, True):
        rec = M.filter_matches(fwd[0], fwd[1], 0.8, cross, rev[0])
        rows = {key(ka[q])[:3] + key(kb[t])[:3] for q, t in zip(rec["query"], rec["train"])}
        assert rec.size > 20 and len(rows) < rec.size
