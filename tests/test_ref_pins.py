"""The CPU oracle against what the reference's OWN prebuilt binary returned (tests/golden/refpin.npz, produced by
tests/golden/make_ref_pins.py through oracle/refexec in the build container).  This is what pins the oracle:
`Sift::calculate` and the `sift::alg` functions of /root/reference/bin/arch_x64/sift, executed in-process, on the
same inputs.  Runs anywhere (the fixture is data); the last test re-runs the binary where the reference is mounted."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from golden_util import read_pgm, sha
from sift_amd.synthetic import blob_frame, synth_frame

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = np.load(os.path.join(HERE, "golden", "refpin.npz"))
import make_ref_pins as G  # noqa: E402  (case tables and image construction, shared with the generator)


def vigra_text(msg: str) -> str:
    """Vigra's what(): leading newline, message, '(header:line)' of the build machine's include path.  The oracle (and the
    product) carry the message proper; file and line are properties of the machine the reference was built on."""
    return re.sub(r"\n\(/[^)]*\)\n+$", "\n", msg.lstrip("\n"))


CALC = sorted(G.CALC_CASES)
HARD = sorted(G.HARD_CASES)       # tests/hard_frames.py's content, pinned in a fixture of its own
HARD_PIN = np.load(G.HARD_PIN)
SCALE = sorted(G.SCALE_CASES)     # scale steps other than sqrt(2): several gradient levels, pinned in a fixture of their own
SCALE_PIN = np.load(G.SCALE_PIN)
ALL_CASES = {**G.CALC_CASES, **G.HARD_CASES, **G.SCALE_CASES}
assert len(ALL_CASES) == len(CALC) + len(HARD) + len(SCALE)


@pytest.mark.parametrize("name", CALC + HARD + SCALE)
def test_calculate_matches_the_reference_binary(name):
    pin = HARD_PIN if name in G.HARD_CASES else SCALE_PIN if name in G.SCALE_CASES else PIN
    spec, dogs, octaves, sub = ALL_CASES[name][:4]
    sigma, k = ALL_CASES[name][4:] if name in G.SCALE_CASES else (1.6, O.K_SQRT2)
    img = G.make_image(spec)
    assert sha(img) == str(pin[f"calc/{name}/image_sha"]), "input differs from the one the reference saw"
    if name in G.SCALE_CASES:
        assert pin[f"calc/{name}/sigma_k"].tobytes() == np.array([sigma, k], np.float32).tobytes()
    run = O.OracleRun(img, dogs, octaves, sigma=sigma, k=k, subpixel=bool(sub))
    if f"calc/{name}/exception" in pin.files:
        assert run.status == 1
        assert vigra_text(run.error).strip() == vigra_text(str(pin[f"calc/{name}/exception"])).strip()
        return
    assert run.status == 0, run.error
    ref = pin[f"calc/{name}/points"]
    got, gdesc = run.points("final")
    assert got.size == ref.size
    for f in ("x", "y", "octave", "index"):
        assert (got[f] == ref[f]).all(), f
    assert (got["filtered"].astype(bool) == ref["filtered"].astype(bool)).all()
    assert got["scale"].tobytes() == ref["scale"].tobytes()
    assert got["orientation"].tobytes() == ref["orientation"].tobytes()
    assert (got["n_desc"] == ref["n_desc"]).all()
    d = np.concatenate([gdesc[i, :got["n_desc"][i]] for i in range(got.size)]) if got.size else np.zeros(0, np.float32)
    assert hashlib.sha256(d.astype(np.float32).tobytes()).hexdigest() == str(pin[f"calc/{name}/desc_sha"])
    # the Gaussian pyramid the reference object kept: Matrix<OctaveElem>(octaves, dogs + 1), element (o, j)
    mw, mh = (int(v) for v in pin[f"calc/{name}/levels_wh"])
    assert (mw, mh) == (octaves, dogs + 1)
    for o in range(mw):
        for j in range(mh):
            lv = run.level("gaussian", o, j)
            k = o * mh + j
            assert tuple(pin[f"calc/{name}/level_dims"][k]) == (lv.shape[1], lv.shape[0])
            assert np.float32(run.scale("gaussian", o, j)).view(np.uint32) == pin[f"calc/{name}/level_scale_bits"][k]
            assert sha(lv) == str(pin[f"calc/{name}/level_sha"][k]), f"gaussian({o},{j})"
    w, h = (int(v) for v in pin[f"calc/{name}/image_dims"])
    assert run.image().shape == (h, w)          # subpixel: the caller's image was replaced (sift.cpp:20-21)
    # the DoG pyramid (Sift::_createDOGs called on its own): Matrix<OctaveElem>(octaves, dogs)
    # (with subpixel, calculate() upsamples before it calls _createDOGs, sift.cpp:20-22: the stand-alone call saw the raw frame)
    dw, dh = (int(v) for v in pin[f"calc/{name}/dogs_wh"])
    assert (dw, dh) == (octaves, dogs)
    for o in range(dw if not sub else 0):
        for j in range(dh):
            lv = run.level("dog", o, j)
            k = o * dh + j
            assert tuple(pin[f"calc/{name}/dog_dims"][k]) == (lv.shape[1], lv.shape[0])
            assert np.float32(run.scale("dog", o, j)).view(np.uint32) == pin[f"calc/{name}/dog_scale_bits"][k]
            assert sha(lv) == str(pin[f"calc/{name}/dog_sha"][k]), f"dog({o},{j})"
    # the gradient maps in their FINAL state: the descriptor stage has added to them in place, keypoint after keypoint.
    # The reference keeps maps of every Gaussian level, the oracle of the levels some keypoint selects.
    checked = 0
    for o in range(mw):
        for j in range(mh):
            for kind, key in (("magnitude", "mag_sha"), ("orientation", "ori_sha")):
                lv = run.level(kind, o, j)
                if lv is not None:
                    assert sha(lv) == str(pin[f"calc/{name}/{key}"][o * mh + j]), f"{kind}({o},{j})"
                    checked += 1
    assert checked >= 2 or ref.size == 0
    if name in G.SCALE_CASES:                   # maps of three and four levels, octave 0's top level among them
        assert checked == 2 * {"synth_160x120_5x2_s0.8_k1.5": 4, "synth_200x150_3x3_s1.0_k1.8": 3}[name]
    if f"calc/{name}/desc" in pin.files:        # the small case stored in full
        assert d.tobytes() == pin[f"calc/{name}/desc"].tobytes()
        flat = np.concatenate([run.level("gaussian", o, j).reshape(-1) for o in range(mw) for j in range(mh)])
        assert flat.tobytes() == pin[f"calc/{name}/levels"].tobytes()


@pytest.mark.parametrize("spec", G.BLUR_IMAGES, ids=[f"{s[1]}x{s[2]}" for s in G.BLUR_IMAGES])
def test_operators_match_the_reference_binary(spec):
    img = G.make_image(spec)
    tag = f"{spec[1]}x{spec[2]}_s{spec[3]}"
    for sigma in G.BLUR_SIGMAS:
        key = f"blur/{tag}/{sigma!r}"
        if key + "/exception" in PIN.files:
            with pytest.raises(O.OracleError) as e:
                O.convolve(img, sigma)
            assert vigra_text(str(e.value.args[-1] if e.value.args else e.value)).strip() in vigra_text(str(PIN[key + "/exception"])).strip() or \
                vigra_text(str(PIN[key + "/exception"])).strip() in str(e.value)
            continue
        assert sha(O.convolve(img, sigma)) == str(PIN[key + "/sha"]), f"convolveWithGauss sigma {sigma}"
    for op, mode in (("reduce", 0), ("increase", 1)):
        out = O.resample(img, 1.6, mode)
        assert tuple(PIN[f"{op}/{tag}/dims"]) == (out.shape[1], out.shape[0])
        assert sha(out) == str(PIN[f"{op}/{tag}/sha"]), op


def test_dog_and_parabola_match_the_reference_binary():
    a, b = synth_frame(200, 150, 3), synth_frame(200, 150, 9)
    out = np.empty_like(a)
    O.lib().oracle_dog(a, b, 200, 150, out)
    assert sha(out) == str(PIN["dog/200x150_s3_s9/sha"])
    L = O.lib()
    L.oracle_vertex_parabola.restype = C.c_float
    L.oracle_vertex_parabola.argtypes = [C.c_uint16, C.c_float, C.c_uint16, C.c_float, C.c_uint16, C.c_float]
    for args, bits in zip(PIN["parabola/args"], PIN["parabola/bits"]):
        r = np.float32(L.oracle_vertex_parabola(int(args[0]), float(args[1]), int(args[2]), float(args[3]), int(args[4]), float(args[5])))
        assert r.view(np.uint32) == bits or (np.isnan(r) and np.isnan(np.uint32(bits).view(np.float32)))


@pytest.mark.skipif(not os.path.exists(G.REF_BIN), reason="the reference is only mounted in the build container")
def test_fixture_is_what_the_reference_binary_returns_now(tmp_path):
    """Live: build oracle/refexec, run the reference's calculate on one case, compare with the committed fixture."""
    root = os.path.dirname(HERE)
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "oracle"), "_ref/refexec"])
    name = "synth_200x160_3x2"
    spec, dogs, octaves, sub = G.CALC_CASES[name]
    r = G.ref_calculate(G.make_image(spec), dogs, octaves, sub, str(tmp_path))
    assert r["points"].tobytes() == PIN[f"calc/{name}/points"].tobytes()
    assert r["desc"].tobytes() == PIN[f"calc/{name}/desc"].tobytes()
    assert r["levels"].tobytes() == PIN[f"calc/{name}/levels"].tobytes()


@pytest.mark.skipif(not os.path.exists(G.REF_BIN), reason="the reference is only mounted in the build container")
@pytest.mark.parametrize("name", HARD)
def test_hard_frame_fixture_is_what_the_reference_binary_returns_now(name, tmp_path):
    """Live, for the frames of tests/hard_frames.py: what the binary returns now against the fixture, and - the fixture keeps
    descriptors and levels as hashes only - against the oracle in full: every point record (several records per keypoint with
    the first peak twice for `signed`, NaN orientations for `binary`), every descriptor float and every Gaussian level."""
    root = os.path.dirname(HERE)
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "oracle"), "_ref/refexec"])
    spec, dogs, octaves, sub = G.HARD_CASES[name]
    img = G.make_image(spec)
    r = G.ref_calculate(img, dogs, octaves, sub, str(tmp_path))
    assert r["points"].tobytes() == HARD_PIN[f"calc/{name}/points"].tobytes()
    assert hashlib.sha256(r["desc"].tobytes()).hexdigest() == str(HARD_PIN[f"calc/{name}/desc_sha"])
    assert list(r["level_sha"]) == [str(v) for v in HARD_PIN[f"calc/{name}/level_sha"]]
    run = O.OracleRun(img, dogs, octaves, subpixel=bool(sub))
    got, gdesc = run.points("final")
    d = _compare_points(got, gdesc, r["points"])
    assert d.tobytes() == r["desc"].tobytes()
    mw, mh = r["levels_wh"]
    flat = np.concatenate([run.level("gaussian", o, j).reshape(-1) for o in range(mw) for j in range(mh)])
    assert flat.tobytes() == r["levels"].tobytes()


# ---- two long-running pins (tens of minutes to hours in the reference: it copies three DoG images per candidate and
# re-blurs a whole level per keypoint); generated once in the build container, skipped when their fixture is absent ----
BENCH_PIN = os.path.join(HERE, "golden", "refpin_bench_frame.npz")
TRUNC_PIN = os.path.join(HERE, "golden", "refpin_u16_truncation.npz")


def _compare_points(got, gdesc, ref):
    assert got.size == ref.size
    for f in ("x", "y", "octave", "index"):
        assert (got[f] == ref[f]).all(), f
    assert got["scale"].tobytes() == ref["scale"].tobytes()
    assert got["orientation"].tobytes() == ref["orientation"].tobytes()
    assert (got["n_desc"] == ref["n_desc"]).all()
    return np.concatenate([gdesc[i, :got["n_desc"][i]] for i in range(got.size)]).astype(np.float32) if got.size else np.zeros(0, np.float32)


@pytest.mark.skipif(not os.path.exists(BENCH_PIN), reason="fixture not generated")
def test_bench_frame_matches_the_reference_binary():
    """Frame 1 of the bench workload itself: 1920x1080, 3 DoGs x 4 octaves (BASELINE.json's metric configuration)."""
    pin = np.load(BENCH_PIN)
    img = synth_frame(1920, 1080, 1)
    assert sha(img) == str(pin["image_sha"])
    run = O.OracleRun(img, 3, 4)
    got, gdesc = run.points("final")
    d = _compare_points(got, gdesc, pin["points"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == str(pin["desc_sha"])
    mw, mh = (int(v) for v in pin["levels_wh"])
    for o in range(mw):
        for j in range(mh):
            assert sha(run.level("gaussian", o, j)) == str(pin["level_sha"][o * mh + j]), f"gaussian({o},{j})"


CONFIG2_PIN = os.path.join(HERE, "golden", "refpin_config2.npz")


@pytest.mark.skipif(not os.path.exists(CONFIG2_PIN), reason="fixture not generated")
def test_config2_as_written_matches_the_reference_binary():
    """BASELINE.json configs[1] exactly as written: one 640x480 frame (seed 1), 4 octaves x 3 DoGs - keypoints, orientations,
    descriptors, every Gaussian and DoG level (octave 3 is 80x60 with radii up to 27, sift.cpp:381-417) and the final gradient
    maps as the reference's own binary returned them."""
    pin = np.load(CONFIG2_PIN)
    dogs, octaves, sub, w, h, seed = (int(v) for v in pin["params"])
    assert (dogs, octaves, sub, w, h, seed) == (3, 4, 0, 640, 480, 1)
    img = synth_frame(w, h, seed)
    assert sha(img) == str(pin["image_sha"])
    run = O.OracleRun(img, dogs, octaves)
    got, gdesc = run.points("final")
    d = _compare_points(got, gdesc, pin["points"])
    assert hashlib.sha256(d.tobytes()).hexdigest() == str(pin["desc_sha"])
    mw, mh = (int(v) for v in pin["levels_wh"])
    for o in range(mw):
        for j in range(mh):
            assert sha(run.level("gaussian", o, j)) == str(pin["level_sha"][o * mh + j]), f"gaussian({o},{j})"
            assert run.scale("gaussian", o, j) == float(np.array(pin["level_scale_bits"][o * mh + j], np.uint32).view(np.float32))
    dw, dh = (int(v) for v in pin["dogs_wh"])
    for o in range(dw):
        for j in range(dh):
            assert sha(run.level("dog", o, j)) == str(pin["dog_sha"][o * dh + j]), f"dog({o},{j})"


@pytest.mark.skipif(not os.path.exists(TRUNC_PIN), reason="fixture not generated")
def test_u16_size_truncation_matches_the_reference_binary():
    """App. B-7 against the reference binary itself: 66260 points survive the first cleanup of this 1024x1088 blob lattice
    (sift_amd.synthetic.blob_frame, seed 5); `u16_t size` (sift.cpp:41) keeps 66260 - 65536 = 724 of them, 720 are returned
    (23 minutes in the reference: it copies three DoG images per candidate)."""
    pin = np.load(TRUNC_PIN)
    w, h, seed = (int(v) for v in pin["params"][3:6])
    img = blob_frame(w, h, seed)
    assert sha(img) == str(pin["image_sha"]) and int(pin["rc"]) == 0
    run = O.OracleRun(img, 3, 4)
    cand, _ = run.points("candidates")
    kept = int((~cand["filtered"].astype(bool)).sum())
    after, _ = run.points("after_sort1")
    assert kept > 65535 and after.size == kept - 65536 == 724
    got, gdesc = run.points("final")
    assert got.size == 720 == pin["points"].size
    d = _compare_points(got, gdesc, pin["points"])
    assert d.tobytes() == pin["desc"].tobytes()


CFG_PIN = os.path.join(HERE, "golden", "refpin_configs_as_written.npz")


@pytest.mark.skipif(not os.path.exists(CFG_PIN), reason="fixture not generated")
@pytest.mark.parametrize("name", ["config3_as_written", "config5_octave5_1792"])
def test_baseline_configs_as_written_end_like_in_the_reference_binary(name):
    """BASELINE.json configs[2] (1080p, subpixel, 4 octaves x 5 DoGs) exactly as written, and configs[4]'s failure mode - the
    dead 16x16 blur of an octave-5 keypoint, sift.cpp:184, App. B-14 - on a frame the reference binary can finish (1792x1792,
    6 octaves x 3 DoGs, no subpixel: 68 minutes; the 4K frame as written would keep it busy for days): what the binary does
    with them is what the oracle does."""
    pin = np.load(CFG_PIN)
    if name + "/rc" not in pin.files:
        pytest.skip("case not in the fixture")
    dogs, octaves, sub, w, h, seed = (int(v) for v in pin[name + "/params"])
    rc, so = int(pin[name + "/rc"]), str(pin[name + "/stdout"])
    assert rc == 5 and so.startswith("EXCEPTION "), "the reference did not throw: regenerate and compare results instead"
    run = O.OracleRun(synth_frame(w, h, seed), dogs, octaves, subpixel=bool(sub))
    assert run.status == 1
    assert vigra_text(run.error).strip() == vigra_text(so[len("EXCEPTION "):]).strip()
