"""Batches in which only SOME images end in the reference's exception (the dead 16x16 blur of App. B-14, sift.cpp:184:
data-dependent and per image), against the CPU oracle run on every frame by itself.  include/sift_hip.h promises that such
an image "has count 0"; everything behind the cleanup has to treat it as an empty set between two full ones: the device-side
scan of output bases and the host's out_base, sift_hip_result_copy, the wire-format counting pass, the offsets of
sift_hip_result_match / _verify, the shards of a group.  A wrong base or offset there hands a caller another image's keypoints
without any error.

The frames are tests/golden/mixed_status_frames.npz (make_mixed_status.py); tests/test_mixed_status_host.py asserts on the CPU
that the "good" ones have keypoints and the "thrown" ones throw.  Every comparison is bitwise.
"""
import functools
import os

import numpy as np
import pytest

import match_ref as M
import oracle_lib as O
import ransac_ref as R
import refine_ref as F
from sift_amd import _lib
from sift_amd.sift import PreconditionViolation, unpack_sparse_host
from test_gpu_parity import _run_isolated, assert_bits_equal, compare_image
from test_mixed_status_host import CONSTANT, GOOD, STAGES, THROWN, load_fixture, oracle_runs
from test_ransac_gpu import _coords, _verify_equals_match_plus_ransac

pytestmark = pytest.mark.gpu

ALL = list(range(7))
PAIRS = [(0, 2), (2, 0), (0, 1), (1, 0), (1, 3), (0, 5), (4, 4), (6, 2), (2, 6)]
EMPTY = (1, 3, 5)


class Mixed:
    """The fixture and the oracle's answer for every frame (one oracle run per frame, shared by every test)."""

    def __init__(self):
        g, prm = load_fixture()
        self.dogs, self.octaves, self.sigma, self.k, self.subpixel = prm
        self.params = _lib.Params(*prm)
        self.u8 = np.ascontiguousarray(g["frames"])
        self.f32 = self.u8.astype(np.float32)
        self.runs = oracle_runs(g, prm)
        self.status = np.array([r.status for r in self.runs])
        self.errors = [r.error for r in self.runs]
        self.final = [r.points("final") for r in self.runs]          # (points, descriptors); empty where it throws
        assert self.status.tolist() == g["status"].tolist() and [i for i in ALL if self.status[i]] == list(THROWN)
        assert all(self.final[i][0].size > 50 for i in GOOD) and self.final[CONSTANT][0].size == 0

    def counts(self, order):
        return [0 if self.status[i] else int(self.final[i][0].size) for i in order]


@functools.lru_cache(maxsize=None)
def mixed_fixture():
    return Mixed()


@pytest.fixture(scope="module")
def mixed():
    return mixed_fixture()


def assert_records(kp, desc, want, wdesc, what):
    """Result records and descriptors against the oracle's final points, field by field, then the descriptor bytes."""
    assert kp.size == want.size and desc.shape == (want.size, 128), f"{what}: {kp.size} records vs oracle {want.size}"
    for f in ("x", "y", "octave", "index"):
        assert (kp[f] == want[f]).all(), f"{what}: field {f} differs at {int((kp[f] != want[f]).sum())} records"
    for f in ("scale", "orientation"):
        assert kp[f].tobytes() == want[f].tobytes(), f"{what}: {f} bit patterns differ"
    assert (kp["has_descriptor"] == (want["n_desc"] == 128)).all(), f"{what}: has_descriptor"
    assert desc.tobytes() == wdesc.tobytes(), f"{what}: descriptors differ in {int((desc != wdesc).sum())} values"


def assert_batch_equals_oracle(mixed, order, status, counts, total, kp, desc, what):
    """status / counts / total / the concatenated results of a batch of frames `order` against the per-image oracle runs."""
    assert status.shape == (len(order),) and ((status != 0) == (mixed.status[order] != 0)).all(), (what, status.tolist())
    assert counts.tolist() == mixed.counts(order), (what, counts.tolist(), mixed.counts(order))
    assert total == sum(mixed.counts(order)) == kp.size, (what, total, kp.size)
    base = 0
    for pos, i in enumerate(order):     # image by image first: a failure names the image
        n = counts[pos]
        if not mixed.status[i]:
            assert_records(kp[base:base + n], desc[base:base + n], *mixed.final[i], f"{what}: image {pos} (F{i})")
        base += n
    good = [i for i in order if not mixed.status[i]]
    want = np.concatenate([mixed.final[i][0] for i in good]) if good else np.zeros(0, O.POINT_DTYPE)
    wdesc = np.concatenate([mixed.final[i][1] for i in good]) if good else np.zeros((0, 128), np.float32)
    assert_records(kp, desc, want, wdesc, what)


def run_batch(ctx, mixed, order, frames=None, raise_on_error=False):
    frames = mixed.f32 if frames is None else frames
    return ctx.calculate_batch(np.ascontiguousarray(frames[order]), mixed.params, raise_on_error=raise_on_error)


def assert_context_holds(ctx, mixed, order, what):
    assert ctx.n_images() == len(order)
    kp, desc = ctx.results()
    assert_batch_equals_oracle(mixed, order, ctx.status(), ctx.counts(), ctx.total(), kp, desc, what)
    return kp, desc


def check_seven_frame_batch(ctx, mixed, what="seven frames", frames=None):
    """Test (a)'s per-image truth for the seven frames in stored order; also what tests/diag_fallbacks.py asserts of the forced
    host path."""
    rc, text = run_batch(ctx, mixed, ALL, frames)
    assert rc == _lib.EPRECONDITION, (what, rc, text)
    assert text == mixed.errors[THROWN[0]] != "", (what, text)        # the first thrown image's
    return assert_context_holds(ctx, mixed, ALL, what)


@pytest.fixture(scope="module")
def alone(ctx, mixed):
    """Every frame that does not throw as a batch of its own: (records, descriptors)."""
    out = {}
    for i in GOOD + (CONSTANT,):
        rc, text = run_batch(ctx, mixed, [i])
        assert rc == _lib.OK and text == "", (i, rc, text)
        out[i] = tuple(a.copy() for a in assert_context_holds(ctx, mixed, [i], f"F{i} alone"))
    return out


def assert_images_equal_alone(ctx, mixed, alone, order, what):
    kp, desc = ctx.results()
    off = np.concatenate([[0], np.cumsum(ctx.counts())])
    assert off[-1] == kp.size
    for pos, i in enumerate(order):
        k, d = kp[off[pos]:off[pos + 1]], desc[off[pos]:off[pos + 1]]
        if mixed.status[i]:
            assert k.size == 0, (what, pos)
        else:
            assert k.tobytes() == alone[i][0].tobytes() and d.tobytes() == alone[i][1].tobytes(), f"{what}: image {pos} (F{i}) differs from F{i} alone"


# ------------------------------------------------------------------------------------------------
def test_one_batch_per_image_truth(ctx, mixed):
    """a. The first batch anywhere in the suite whose images differ in status: the status[img*4 + 0..3] handling of mid_gpu,
    desc_grid_kernel's scan of output bases with zeros in the middle, sift_hip_result_copy over them; every stage list and every
    level of every image.  A thrown image keeps what the reference had formed when it threw (include/sift_hip.h)."""
    check_seven_frame_batch(ctx, mixed)
    for i in ALL:
        run = mixed.runs[i]
        if not mixed.status[i]:
            rep = {}
            compare_image(ctx, run, i, mixed.dogs, mixed.octaves, False, f"mixed batch F{i}", rep)
            assert rep["final"] == mixed.counts([i])[0]
            continue
        assert ctx.stage("final", i).size == 0 and ctx.counts()[i] == 0
        # the reference threw inside _orientationAssignment: the lists formed until then are the oracle's, the later ones empty
        for stage in STAGES:
            got, want = ctx.stage(stage, i), run.points(stage)[0]
            assert got.size == want.size, f"thrown F{i}: {stage}: {got.size} points vs oracle {want.size}"
            for f in ("x", "y", "octave", "index"):
                assert (got[f] == want[f]).all(), f"thrown F{i}: {stage}: field {f}"
            assert got["scale"].tobytes() == want["scale"].tobytes(), f"thrown F{i}: {stage}: scale"
        assert ctx.stage("after_sort1", i).size > 0 and ctx.stage("after_orient", i).size == 0 and ctx.stage("after_sort2", i).size == 0
        cand, wcand = ctx.stage("candidates", i), run.points("candidates")[0]
        assert (cand["filtered"].astype(bool) == wcand["filtered"].astype(bool)).all(), f"thrown F{i}: candidate flags"
        for o in range(mixed.octaves):
            for j in range(mixed.dogs + 1):
                assert_bits_equal(ctx.level("gaussian", o, j, i), run.level("gaussian", o, j), f"thrown F{i}: gaussian({o},{j})")
            for j in range(mixed.dogs):
                assert_bits_equal(ctx.level("dog", o, j, i), run.level("dog", o, j), f"thrown F{i}: dog({o},{j})")


@pytest.mark.parametrize("order", [[1, 0, 2], [0, 2, 3], [1, 3], [0, 2, 4, 6]], ids=["thrown first", "thrown last", "all thrown", "none thrown"])
def test_position_independence(ctx, mixed, alone, order):
    """b. Wherever the thrown image stands, each good image's records and descriptors are those of the same image alone."""
    rc, text = run_batch(ctx, mixed, order)
    thrown = [i for i in order if mixed.status[i]]
    if thrown:
        assert rc == _lib.EPRECONDITION and text == mixed.errors[thrown[0]]
    else:
        assert rc == _lib.OK and text == "" and (ctx.status() == 0).all()
    kp, desc = assert_context_holds(ctx, mixed, order, str(order))
    assert_images_equal_alone(ctx, mixed, alone, order, str(order))
    if len(thrown) == len(order):
        assert ctx.total() == 0 and kp.size == 0 and desc.shape == (0, 128)
        rec, val = ctx.results_sparse()
        assert rec.shape == (0, 34) and val.size == 0 and unpack_sparse_host(rec, val)[0].size == 0
        for i in range(len(order)):
            assert ctx.stage("final", i).size == 0


def test_raising_path_keeps_the_batch_readable(ctx, mixed):
    """c. The default raise_on_error=True: the exception carries the oracle's text, and the batch's results stay readable."""
    with pytest.raises(PreconditionViolation) as e:
        run_batch(ctx, mixed, ALL, raise_on_error=True)
    assert str(e.value) == mixed.errors[THROWN[0]]
    assert ctx.n_images() == 7
    assert_context_holds(ctx, mixed, ALL, "after the exception")


def test_no_state_leaks_into_the_next_batch(ctx, mixed, alone):
    """d. mixed, then a clean batch on the same context (status and messages of the batch before must be gone), then mixed."""
    check_seven_frame_batch(ctx, mixed, "first mixed batch")
    rc, text = run_batch(ctx, mixed, [0, 2])
    assert rc == _lib.OK and text == "" and ctx.status().tolist() == [0, 0]
    assert_context_holds(ctx, mixed, [0, 2], "clean batch after a mixed one")
    assert_images_equal_alone(ctx, mixed, alone, [0, 2], "clean batch after a mixed one")
    check_seven_frame_batch(ctx, mixed, "second mixed batch")


def test_sparse_lists(ctx, mixed):
    """e. The wire-format counting pass over a batch with empty sets in the middle: as a pass of its own, and riding in the
    descriptor kernel (option wire_count)."""
    sizes = []
    for wire_count in (0, 1):
        ctx.set_option("wire_count", wire_count)
        try:
            kp, desc = check_seven_frame_batch(ctx, mixed, f"wire_count {wire_count}")
            nnz = ctx.sparse_size()                              # raises unless the format is lossless for these results
            assert nnz == int((desc.view(np.uint32) != 0).sum())
            sizes.append(nnz)
            sparse = ctx.results_sparse()
            assert sparse is not None
            rec, val = sparse
            assert rec.shape == (kp.size, 34) and val.size == nnz
            for threads in (1, 5):
                kp2, desc2 = unpack_sparse_host(rec, val, threads=threads)
                assert kp2.tobytes() == kp.tobytes() and desc2.tobytes() == desc.tobytes(), (wire_count, threads)
        finally:
            ctx.set_option("wire_count", 0)
    assert sizes[0] == sizes[1] > 0


def test_u8_entry(ctx, mixed):
    """f. The stored 8-bit frames through sift_hip_calculate_batch_u8: statuses, counts and result bytes of their float form."""
    kp, desc = (a.copy() for a in check_seven_frame_batch(ctx, mixed, "float frames"))
    status, counts = ctx.status().copy(), ctx.counts().copy()
    assert mixed.u8.dtype == np.uint8
    kp8, desc8 = check_seven_frame_batch(ctx, mixed, "uint8 frames", frames=mixed.u8)
    assert ctx.status().tolist() == status.tolist() and ctx.counts().tolist() == counts.tolist()
    assert kp8.tobytes() == kp.tobytes() and desc8.tobytes() == desc.tobytes()


def _expected_matches(kp, desc, cnt, pairs, ratio, cross):
    off = np.concatenate([[0], np.cumsum(cnt)])
    sets = [desc[off[i]:off[i + 1]] for i in range(cnt.size)]
    valid = [kp["has_descriptor"][off[i]:off[i + 1]] for i in range(cnt.size)]
    want = []
    for a, b in pairs:
        fwd = M.knn2(sets[a], sets[b], valid[a], valid[b])
        rev = M.knn2(sets[b], sets[a], valid[b], valid[a])
        want.append(M.filter_matches(fwd[0], fwd[1], ratio, cross, rev[0]))
    return want


def test_match_and_verify_on_device_results(ctx, mixed):
    """g. sift_hip_result_match / sift_hip_result_verify over v.counts with empty sets (thrown images and the constant one) and a
    pair with the same image on both sides: the offsets match_result_on_device builds.  No geometric assertion: the images
    differ, only the equality with the host loops counts."""
    kp, desc = (a.copy() for a in check_seven_frame_batch(ctx, mixed))
    cnt = ctx.counts().copy()
    off = np.concatenate([[0], np.cumsum(cnt)])
    empty_pairs = [p for p, (a, b) in enumerate(PAIRS) if a in EMPTY or b in EMPTY]
    assert empty_pairs == [2, 3, 4, 5]
    for ratio, cross in ((0.8, False), (0.8, True), (0.0, False)):
        rec, counts = ctx.match_images(PAIRS, ratio, cross)
        want = _expected_matches(kp, desc, cnt, PAIRS, ratio, cross)
        print(f"ratio {ratio} cross {cross}: {counts.tolist()} matches")
        assert counts.tolist() == [w.size for w in want], (ratio, cross)
        assert M.same_bits(rec.astype(want[0].dtype), np.concatenate(want)), (ratio, cross)
        assert (counts[empty_pairs] == 0).all()
        roff = np.concatenate([[0], np.cumsum(counts)])
        own = rec[roff[6]:roff[7]]                                # (4, 4): every valid row finds itself at distance 0
        valid = kp["has_descriptor"][off[4]:off[5]].astype(bool)
        assert (own["dist2"] == 0).all()                          # d2(a, a) == 0 and no d2 is below 0
        if ratio == 0:
            assert own.size == int(valid.sum()) > 50 and (own["query"] == np.nonzero(valid)[0]).all()
            assert (own["train"] == own["query"]).all()          # no two rows of F4 are equal (the host checker on the oracle's rows)
            assert (desc[off[4]:off[5]][own["train"]] == desc[off[4]:off[5]][own["query"]]).all()   # itself, or a row equal to it in front
    # the geometric check of the same lists
    rec, counts, models, flags = _verify_equals_match_plus_ransac(ctx, kp, cnt, PAIRS, 0.8, False, 256, 1, 1.0)
    assert (models["refined"] == 0).all()
    got = ctx.verify_images(PAIRS, 0.8, False, 256, 3.0, 1, refine=2)
    assert R.same_bits(got[0], rec) and R.same_bits(got[1], counts) and got[3].size == rec.size
    roff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.zeros((rec.size, 4), np.float32)
    for p, (a, b) in enumerate(PAIRS):
        r = rec[roff[p]:roff[p + 1]]
        pts[roff[p]:roff[p + 1]] = np.concatenate([_coords(kp, cnt, a, r["query"], 1.0), _coords(kp, cnt, b, r["train"], 1.0)], axis=1)
    want = F.ransac(pts, roff, 256, 3.0, 1, refine=2)
    assert np.asarray(got[2]).tobytes() == want[0].tobytes() and R.same_bits(got[3], want[1])
    dev = ctx.ransac_homography(pts, roff, 256, 3.0, 1, refine=2)
    assert np.asarray(dev[0]).tobytes() == want[0].tobytes() and R.same_bits(dev[1], want[1])
    for m in (models, got[2]):
        for p in empty_pairs:
            assert counts[p] == 0 and m["iteration"][p] == -1 and m["inliers"][p] == 0 and m["refined"][p] == 0
            assert m["h"][p].tobytes() == bytes(36)                # all +0.0f
    assert flags.size == rec.size == int(counts.sum())             # an empty pair owns no flag


_GROUP_MIXED_SCRIPT = """
import os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(O.__file__)), "golden"))     # as tests/conftest.py does
import test_mixed_status_gpu as T
mixed = T.mixed_fixture()
g = Group([0, 0, 0])                                   # 7 frames over 3 shards: F0 F1 F2 | F3 F4 F5 | F6
rc, text = g.calculate_batch(mixed.f32, mixed.params, raise_on_error=False)
assert rc == _lib.EPRECONDITION and text == mixed.errors[1], (rc, text)
kp, desc = g.results()
T.assert_batch_equals_oracle(mixed, T.ALL, g.status(), g.counts(), g.total(), kp, desc, "group of three shards")
ctx = Context(0)
wkp, wdesc = T.check_seven_frame_batch(ctx, mixed, "single context")
assert g.status().tolist() == ctx.status().tolist() and g.counts().tolist() == ctx.counts().tolist() and g.total() == ctx.total()
assert kp.tobytes() == wkp.tobytes() and desc.tobytes() == wdesc.tobytes()
with pytest.raises(PreconditionViolation) as e:
    g.calculate_batch(mixed.f32, mixed.params)
assert str(e.value) == mixed.errors[1]
g.close(); ctx.close()
print("isolated ok")
"""


def test_group_of_shards(mixed):
    """h. A group of three shards on device 0 over the seven frames (a thrown image in the middle of the first shard, at the
    head of the second): the per-image bookkeeping of group.cpp and its gather with empty lists, against the single context and
    the oracle.  (In a process of its own: test_gpu_parity._run_isolated.)"""
    _run_isolated(_GROUP_MIXED_SCRIPT, timeout=600)
