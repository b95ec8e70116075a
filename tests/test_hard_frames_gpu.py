"""The frames of tests/hard_frames.py through the HIP path, bit for bit against the CPU oracle (which stands on the reference's
binary for four of them: tests/test_ref_pins.py; tests/test_hard_frames_host.py holds the property that makes each frame hard).

What only these frames reach: a keypoint with several orientation peaks (`signed`) makes the GPU path of the middle stages
give up after its speculative descriptor stage - mid_gpu returns false, context.cpp - and the WHOLE batch is redone by
mid_host: peaks copied to the host, one record appended per peak, a second descriptor launch over records that share their
coordinates.  `binary` has NaN orientations, which the descriptor stage adds into its per-pixel chains, and all-zero
descriptors; the others tie on plateaus and mirror axes or fill the candidate lists with points that are all filtered."""
import functools

import numpy as np
import pytest

import fund_ref as F
import oracle_lib as O
import ransac_ref as R
from hard_frames import CASES, case_id, hard_frame, signed
from sift_amd import _lib
from sift_amd.sift import unpack_sparse_host
from sift_amd.synthetic import synth_frame
from test_gpu_parity import compare_image, compare_run
from test_mixed_status_gpu import _expected_matches
from test_mixed_status_gpu import assert_records as assert_records_bytes
from test_ransac_gpu import _coords, _verify_equals_match_plus_ransac

pytestmark = pytest.mark.gpu

W, H, DOGS, OCTAVES = 160, 120, 3, 2


def params(dogs=DOGS, octaves=OCTAVES, subpixel=False):
    return _lib.Params(dogs, octaves, 1.6, O.K_SQRT2, 1 if subpixel else 0)


def fell_back(ctx, image=0):
    """More records behind the orientation stage than in front of it: some keypoint had several peaks, which the GPU path of
    the middle stages hands to mid_host (context.cpp: mid_gpu's return false) - the proof that the fallback ran."""
    return ctx.stage("after_orient", image).size > ctx.stage("after_sort1", image).size


def assert_records(kp, desc, want, wdesc, what):
    """test_mixed_status_gpu.assert_records (fields, then scale, orientation and descriptors by bytes) with one NaN for all:
    the sign bit of the x86 default NaN the oracle returns (App. B-9, h0 = 0) is not the GPU's."""
    kp, want = kp.copy(), want.copy()
    for a in (kp, want):
        a["orientation"][np.isnan(a["orientation"])] = np.float32("nan")
    assert_records_bytes(kp, desc, want, wdesc, what)


def snapshot(ctx):
    kp, desc = ctx.results()
    return ctx.counts().copy(), kp.copy(), desc.copy()


def same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# the frames of the batches of c, d and f: name -> image, all W x H
@functools.lru_cache(maxsize=None)
def frame(name):
    kind, _, seed = name.partition(":")
    if kind == "synth":
        return synth_frame(W, H, int(seed))
    if kind == "const":
        return np.full((H, W), float(seed), np.float32)
    return hard_frame(kind, W, H, int(seed) if seed else None)


@functools.lru_cache(maxsize=None)
def oracle_final(name, dogs=DOGS, octaves=OCTAVES):
    run = O.OracleRun(frame(name), dogs, octaves)
    assert run.status == 0, run.error
    return run.points("final")


@pytest.fixture(scope="module")
def alone(ctx):
    """name -> (counts, records, descriptors) of the frame as a batch of its own, checked against the oracle; computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            ctx.calculate_batch(frame(name)[None], params())
            cache[name] = snapshot(ctx)
            assert_records(cache[name][1], cache[name][2], *oracle_final(name), f"{name} alone")
            assert fell_back(ctx) == name.startswith("signed"), name
        return cache[name]
    return get


def assert_images_equal_alone(ctx, alone, names, what):
    got = snapshot(ctx)          # before `alone` runs batches of its own on the same context
    off = np.concatenate([[0], np.cumsum(got[0])])
    assert off[-1] == got[1].size == ctx.total()
    for pos, name in enumerate(names):
        want = alone(name)
        assert got[0][pos] == want[0][0], f"{what}: image {pos} ({name}): count {got[0][pos]} vs {want[0][0]} alone"
        assert got[1][off[pos]:off[pos + 1]].tobytes() == want[1].tobytes(), f"{what}: image {pos} ({name}): records differ from the frame alone"
        assert got[2][off[pos]:off[pos + 1]].tobytes() == want[2].tobytes(), f"{what}: image {pos} ({name}): descriptors differ from the frame alone"


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_hard_frame_parity(ctx, report_dir, case):
    """a. Every level, the five stage lists, orientations (NaN equals NaN), descriptors by bytes and has_descriptor."""
    kind, w, h, dogs, octaves, sub = case
    rep = compare_run(ctx, hard_frame(kind, w, h), dogs, octaves, sub, "hard frame " + case_id(case), report_dir)
    assert fell_back(ctx) == (kind == "signed")
    if kind == "signed":
        assert rep["after_orient"] > rep["after_sort1"]
    if kind in ("stripes", "unit"):
        assert rep["candidates"] > 1000 and rep["final"] == 0 and ctx.total() == 0
    else:
        assert rep["final"] >= 20
    if kind == "binary":
        kp, desc = ctx.results()
        assert np.isnan(kp["orientation"]).any() and (kp["has_descriptor"].astype(bool) & (desc == 0).all(axis=1)).any()


def test_signed_batch_of_three(ctx, report_dir):
    """b. The redo over a batch of several images that all need it."""
    compare_run(ctx, hard_frame("signed", W, H), DOGS, OCTAVES, False, "signed x3", report_dir, batch_of=3)
    assert all(fell_back(ctx, i) for i in range(3))


def test_signed_with_general_orientation_bins(ctx, report_dir):
    """b. The histogram's per-sample-bin form finds the same peaks."""
    ctx.set_option("orient_general", 1)
    try:
        compare_run(ctx, hard_frame("signed", W, H), DOGS, OCTAVES, False, "signed, general orientation bins", report_dir, batch_of=2)
        assert fell_back(ctx, 0) and fell_back(ctx, 1)
    finally:
        ctx.set_option("orient_general", 0)


MIXED_ORDERS = {
    "signed in the middle": ["synth:1", "signed", "binary", "const:7", "synth:2"],
    "signed first": ["signed", "synth:1", "binary", "const:7", "synth:2"],
    "signed last": ["synth:1", "binary", "const:7", "synth:2", "signed"],
}


@pytest.mark.parametrize("order", list(MIXED_ORDERS), ids=list(MIXED_ORDERS))
def test_mixed_batch_equals_each_image_alone(ctx, alone, order):
    """c. One image with several peaks sends the whole batch through mid_host: the ordinary, the NaN-orientation and the
    constant image beside it must come out as from batches of their own (which took the GPU path)."""
    names = MIXED_ORDERS[order]
    imgs = np.stack([frame(n) for n in names])
    rc, text = ctx.calculate_batch(imgs, params())
    assert rc == _lib.OK and text == "" and (ctx.status() == 0).all()
    assert [fell_back(ctx, i) for i in range(len(names))] == [n == "signed" for n in names]
    assert ctx.counts()[names.index("const:7")] == 0
    for pos, name in enumerate(names):     # stage lists and levels of every image, straight against the oracle
        run = O.OracleRun(frame(name), DOGS, OCTAVES)
        compare_image(ctx, run, pos, DOGS, OCTAVES, False, f"{order}: image {pos} ({name})", {})
    assert_images_equal_alone(ctx, alone, names, order)


def test_no_state_survives_a_redone_batch(ctx, report_dir):
    """d. ordinary, signed, ordinary, signed of another size on one context: `described`, `wire_counted`, `stages_on_host`, the
    host's peaks and the device's stale peaks of one batch must not reach the next."""
    ordinary = np.stack([frame("synth:1"), frame("synth:2")])
    ctx.calculate_batch(ordinary, params())
    first = snapshot(ctx)
    first_stages = [ctx.stage(s, 1).tobytes() for s in O.OracleRun.STAGES]
    assert first[0].min() > 0 and not fell_back(ctx, 0) and not fell_back(ctx, 1)
    ctx.calculate_batch(np.stack([frame("signed"), frame("signed:5"), frame("signed:6")]), params())
    assert all(fell_back(ctx, i) for i in range(3))
    for i, name in enumerate(("signed", "signed:5", "signed:6")):
        off = int(ctx.counts()[:i].sum())
        kp, desc = ctx.results()
        assert_records(kp[off:off + ctx.counts()[i]], desc[off:off + ctx.counts()[i]], *oracle_final(name), f"second batch: {name}")
    ctx.calculate_batch(ordinary, params())
    assert same(snapshot(ctx), first), "the ordinary batch after a redone one differs from the same batch before it"
    assert [ctx.stage(s, 1).tobytes() for s in O.OracleRun.STAGES] == first_stages
    assert not fell_back(ctx, 0) and not fell_back(ctx, 1)
    compare_run(ctx, hard_frame("signed", 192, 144, 7), 3, 3, False, "signed 192x144 x2 after an ordinary batch", report_dir, batch_of=2)
    assert fell_back(ctx, 0) and fell_back(ctx, 1)


def sparse_round_trip(ctx, kp, desc, lossless):
    """sift_hip_result_sparse_size / _pack / sift_hip_sparse_unpack and sift_hip_result_copy_sparse / sift_hip_sparse_unpack_host
    over the context's current results, against the torch restatement of the wire format (sift_amd/gather.py) applied to the
    dense result (kp, desc).  The format carries the 112 informative floats of a descriptor; with `lossless` the round trip must
    return the dense result, without it the dense result with +0.0f in bin 7 of every cell (include/sift_hip.h)."""
    import torch
    from sift_amd.gather import join_records, pack_sparse, split_records, unpack_sparse
    total = ctx.total()
    assert total == kp.size
    carried = np.ascontiguousarray(desc.reshape(-1, 16, 8)[:, :, :7])
    back = desc.reshape(-1, 16, 8).copy()
    back[:, :, 7] = 0.0
    back = back.reshape(-1, 128)
    assert (back.tobytes() == desc.tobytes()) == lossless
    nnz = ctx.sparse_size(require_lossless=False)
    assert nnz == int((carried.view(np.uint32) != 0).sum())
    if lossless:
        assert ctx.sparse_size() == nnz
    else:
        with pytest.raises(ValueError):
            ctx.sparse_size()
        assert ctx.results_sparse() is None
    masks_ref, values_ref = pack_sparse(torch.from_numpy(desc.reshape(-1)))
    rec_ref = join_records(torch.from_numpy(kp.view(np.uint8).reshape(-1)), masks_ref)
    assert values_ref.numel() == nnz
    rec = torch.full((total * 34,), 0xCD, dtype=torch.uint8, device="cuda:0")
    values = torch.full((nnz,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sparse_pack(rec.data_ptr(), values.data_ptr())                                    # sift_hip_result_sparse_pack
    assert rec.cpu().numpy().tobytes() == rec_ref.numpy().tobytes()
    assert values.cpu().numpy().tobytes() == values_ref.numpy().tobytes()
    recs, masks = split_records(rec.cpu())
    assert recs.numpy().tobytes() == kp.tobytes()
    assert unpack_sparse(masks, values.cpu()).numpy().tobytes() == back.tobytes()
    kp_dev = torch.full((total * 20,), 0xAB, dtype=torch.uint8, device="cuda:0")
    desc_dev = torch.full((total * 128,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sparse_unpack(rec.data_ptr(), values.data_ptr(), total, kp_dev.data_ptr(), desc_dev.data_ptr())
    assert kp_dev.cpu().numpy().tobytes() == kp.tobytes() and desc_dev.cpu().numpy().tobytes() == back.tobytes()
    hrec, hval = np.full((total, 34), 0xEE, np.uint8), np.full(nnz, np.nan, np.float32)
    assert ctx._L.sift_hip_result_copy_sparse(ctx._h, hrec.ctypes.data, hval.ctypes.data) == _lib.OK
    assert hrec.tobytes() == rec_ref.numpy().tobytes() and hval.tobytes() == values_ref.numpy().tobytes()
    if lossless:
        lrec, lval = ctx.results_sparse()
        assert lrec.tobytes() == hrec.tobytes() and lval.tobytes() == hval.tobytes()
    for threads in (1, 5):
        kp2, desc2 = unpack_sparse_host(hrec, hval, threads=threads)
        assert kp2.tobytes() == kp.tobytes() and desc2.tobytes() == back.tobytes()


@pytest.mark.parametrize("wire_count", [0, 1])
def test_sparse_lists_after_a_redone_batch(ctx, wire_count):
    """e. The speculative descriptor stage's wire counts are discarded with it: the sizes, the packed lists and both unpacking
    sides must be those of the redone batch's dense result, counted again.

    The round trip as far as the format goes: a cell whose bin sum is negative - zero-mean pixels weight the samples with a
    negative Gaussian pixel value - is normalised to -0.0f in its never-written bin 7 (4627 of the oracle's 5344 cells on the
    160x120 frame; the reference's own binary returns the same descriptors).  The wire format does not carry bin 7, and
    sift_hip_result_sparse_size must say so (lossless = 0, include/sift_hip.h); every float it does carry, the records and the
    sizes are compared bit for bit, bin 7 comes back +0.0f.  The ordinary batch behind it on the same context is lossless
    again and makes the whole round trip to its dense result."""
    imgs = np.stack([frame("signed"), frame("synth:1"), frame("signed:5")])
    ordinary = np.stack([frame("synth:1"), frame("const:7"), frame("synth:2")])
    ctx.set_option("wire_count", wire_count)
    try:
        ctx.calculate_batch(imgs, params())
        assert fell_back(ctx, 0) and not fell_back(ctx, 1) and fell_back(ctx, 2)
        kp, desc = ctx.results()
        assert kp.size > 300
        for i, name in enumerate(("signed", "synth:1", "signed:5")):
            off = int(ctx.counts()[:i].sum())
            assert_records(kp[off:off + ctx.counts()[i]], desc[off:off + ctx.counts()[i]], *oracle_final(name), f"wire_count {wire_count}: {name}")
        assert (desc.reshape(-1, 16, 8)[:, :, 7].view(np.uint32) == 0x80000000).any()
        sparse_round_trip(ctx, kp, desc, lossless=False)
        ctx.calculate_batch(ordinary, params())
        kp, desc = ctx.results()
        assert kp.size > 100 and ctx.counts()[1] == 0 and not fell_back(ctx, 0)
        sparse_round_trip(ctx, kp, desc, lossless=True)
    finally:
        ctx.set_option("wire_count", 0)


def test_run_stream_with_a_redone_batch_in_the_middle(ctx):
    """f. Two gated contexts take batches from one source; the `signed` batch in the middle is redone on the host while its
    neighbours run.  The redo passes no gate (PhaseGate::mark is idempotent, before_descriptors is not called again): its
    descriptor stage runs after phase D was signalled, which costs order only.  Every batch equals the single ungated context."""
    from sift_amd.pipeline import BatchPipeline
    prm = params()
    names = [[f"synth:{300 + 3 * b + i}" for i in range(3)] for b in range(7)]
    names[3] = ["signed", "signed:5", "signed:6"]
    batches = [np.stack([frame(n) for n in b]) for b in names]
    got = {}
    with BatchPipeline(0, depth=2) as pipe:
        it = iter(range(len(batches)))

        def source():
            b = next(it, None)
            return None if b is None else (batches[b], prm)

        def sink(c, slot, item):
            b = next(i for i, a in enumerate(batches) if a is item[0])
            got[b] = (slot, fell_back(c, 0)) + snapshot(c)

        pipe.run_stream(source, sink)
    assert sorted(got) == list(range(7)) and {got[b][0] for b in got} == {0, 1}
    assert [got[b][1] for b in range(7)] == [b == 3 for b in range(7)]
    for b in range(7):
        ctx.calculate_batch(batches[b], prm)
        assert same(got[b][2:], snapshot(ctx)), f"batch {b} differs from the single context's"
        assert got[b][2].min() > 0


def test_match_and_verify_signed_views(ctx):
    """g. Two views of one `signed` frame 8 columns apart: the result lists hold several records per keypoint location (one
    per peak), so a RANSAC sample can draw rows with equal coordinates - the degenerate samples of ransac_math.h and
    ransac_fund_math.h.  sift_hip_result_match / _verify (homography and fundamental) against the host checkers, bitwise."""
    big = signed(272, 192, 1)
    imgs = np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])])
    ctx.calculate_batch(imgs, params(3, 3))
    assert fell_back(ctx, 0) and fell_back(ctx, 1)
    kp, desc = (a.copy() for a in ctx.results())
    cnt = ctx.counts().copy()
    for i in range(2):
        want, wdesc = O.OracleRun(imgs[i], 3, 3).points("final")
        k = kp[cnt[:i].sum():cnt[:i + 1].sum()]
        assert_records(k, desc[cnt[:i].sum():cnt[:i + 1].sum()], want, wdesc, f"view {i}")
        loc = np.stack([k["x"], k["y"], k["octave"], k["index"]], axis=1)
        assert np.unique(loc, axis=0).shape[0] < k.size - 50          # records that share their coordinates
    pairs = [(0, 1), (1, 0)]
    for cross in (False, True):
        rec, counts = ctx.match_images(pairs, 0.8, cross)
        want = _expected_matches(kp, desc, cnt, pairs, 0.8, cross)
        assert counts.tolist() == [w.size for w in want] and counts.min() > 20, (cross, counts.tolist())
        assert rec.astype(want[0].dtype).tobytes() == np.concatenate(want).tobytes(), cross
        # homography: sift_hip_result_verify = the match lists + the host loop on their coordinates
        rec_h, counts_h, models, flags = _verify_equals_match_plus_ransac(ctx, kp, cnt, pairs, 0.8, cross, 512, 19, 1.0)
        assert R.same_bits(rec_h, rec) and (models["iteration"] >= 0).all()
        # fundamental
        rec_f, counts_f, fm, fflags = ctx.verify_images(pairs, 0.8, cross, 512, 1.0, 19, model="fundamental")
        assert fm.dtype == _lib.FUNDAMENTAL_DTYPE and F.same_bits(rec_f, rec) and F.same_bits(counts_f, counts) and fflags.size == rec.size
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.zeros((rec.size, 4), np.float32)
        for p, (a, b) in enumerate(pairs):
            r = rec[off[p]:off[p + 1]]
            pts[off[p]:off[p + 1]] = np.concatenate([_coords(kp, cnt, a, r["query"], 1.0), _coords(kp, cnt, b, r["train"], 1.0)], axis=1)
        assert np.unique(pts[off[0]:off[1]], axis=0).shape[0] < counts[0]      # equal rows a sample can draw twice
        host = F.ransac(pts, off, 512, 1.0, 19)
        assert fm.astype(F.MODEL_DTYPE).tobytes() == host[0].tobytes() and F.same_bits(fflags, host[1])
        dev = ctx.ransac_fundamental(pts, off, 512, 1.0, 19)
        assert F.same_bits(fm, dev[0]) and F.same_bits(fflags, dev[1])
