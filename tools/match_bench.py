"""Descriptor matching on the GPU, measured (bench.py measures extraction and is left alone).

Cases: (a) frames 1 and 2 of the bench batch (about 19.7 k rows each), the top-2 on the pipeline's device-resident
descriptors; (b) the 31 consecutive pairs of the 32-frame bench batch in ONE sift_hip_result_match call; (c) the 444 x 441
pair of the tests.  Comparator, same GPU, same data, alternating with the fused arm in the same run: the torch formulation
nq[:, None] + nt[None, :] - 2 * q @ t.T, then topk(2, largest=False) - which writes and re-reads the nq x nt matrix.

Timing: a warm-up, then --reps repetitions of each arm in turn; median and min - max.  The library's calls run on the context's
own stream and return when the result is in place, so the fused arm is timed on the host around the call (perf_counter: the
GPU time plus the launch and the wait, an upper bound); the torch arm is timed the same way around a synchronize, and with HIP
events as well.  Achieved TF/s = 2 * nq * nt * 128 / time, beside the 157.3 TF f32 matrix peak of the MI355X and the 122 TF of
an untuned f32 MFMA GEMM.  On (a), 256 sampled query rows are compared bit for bit with the host checker.

    python tools/match_bench.py [--reps 20] [--frames 32] [--out profiles/match_bench.txt]

--guided-arm: guided matching instead (no torch arm).  On cases (a) and (b), without and with the cross-check, and for both
models, sift_hip_result_match alternates with sift_hip_result_match_guided under (1) the models of a preceding verify_images at
3 px, (2) a model and a threshold that admit every row (the early skip of the tile kernel works as in the unguided kernel) and
(3) a band of 3 px under a fixed model (nearly every candidate is inadmissible, a lane's second best stays +inf for long).  The
frames of the bench batch are unrelated, so (1) is a narrow band too.  Median, min and max of --reps; lines are appended to
--out.  --unguided-only: the unguided calls of those cases alone (for an A/B of two builds, SIFT_HIP_LIBRARY).

--u8-arm: 8-bit descriptors and integer matching beside the float matcher (no torch arm), alternating in the same run: the top-2
of case (a) on device-resident rows (sift_hip_knn2 on the float results against sift_hip_knn2_u8 on their bytes), and case (b)
without and with the cross-check (sift_hip_result_match with quantized = 0 against quantized = 1, which includes the quantiser's
pass).  256 sampled query rows of (a) are compared bit for bit with the integer host checker.  Median, min and max of --reps, the
ratio of the medians, and whether the two min - max intervals overlap (then there is no winner); lines are appended to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--guided-arm", action="store_true")
    ap.add_argument("--unguided-only", action="store_true")
    ap.add_argument("--u8-arm", action="store_true")
    args = ap.parse_args()

    import torch
    import match_ref as M
    from sift_amd import _lib
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_batch, synth_frame

    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def torch_top2(q, t):
        nq, nt = (q * q).sum(dim=1), (t * t).sum(dim=1)
        d = nq[:, None] + nt[None, :] - 2.0 * (q @ t.T)
        return torch.topk(d, min(2, t.shape[0]), dim=1, largest=False)

    def race(fused, comparator, flop):
        """Alternate the two arms; host time of both, event time of the torch arm."""
        for _ in range(args.warmup):
            fused()
            comparator()
        torch.cuda.synchronize()
        f_ms, t_ms, t_ev = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fused()
            f_ms.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            comparator()
            e1.record()
            torch.cuda.synchronize()
            t_ms.append((time.perf_counter() - t0) * 1e3)
            t_ev.append(e0.elapsed_time(e1))
        f, t = stats(f_ms), stats(t_ms)
        return {"fused": f, "torch": t, "torch_events": stats(t_ev), "fused_tflops": round(flop / (f["median_ms"] * 1e-3) / 1e12, 2),
                "torch_tflops": round(flop / (t["median_ms"] * 1e-3) / 1e12, 2), "speedup_vs_torch": round(t["median_ms"] / f["median_ms"], 2),
                "f32_matrix_peak_tflops": 157.3, "untuned_mfma_gemm_tflops": 122}

    def timed(arms):
        """Alternate the arms (name -> call); host time around each call."""
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        ms = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        return {k: stats(v) for k, v in ms.items()}

    def guided_arms(ctx, cnt):
        identity = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
        f_all = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)            # a = 1, b = 0: g > 0 at every row
        f_rows = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)          # epipolar lines ty = qy
        n = cnt.size
        for name, pairs in (("a: frames 1 and 2", [(0, 1)]), (f"b: the {n - 1} consecutive pairs", [(i, i + 1) for i in range(n - 1)])):
            for cross in (False, True):
                arms = {"unguided": lambda: ctx.match_images(pairs, 0.8, cross)}
                if args.unguided_only:
                    emit({"case": name, "cross_check": cross, "library": os.path.basename(_lib.LIB_PATH), **timed(arms)})
                    continue
                found = {}
                for kind, every, fixed in (("homography", identity, identity), ("fundamental", f_all, f_rows)):
                    models = ctx.verify_images(pairs, 0.8, cross, 512, 3.0, 0, model=kind)[2]
                    tile = lambda m: np.tile(m, (len(pairs), 1))   # noqa: E731
                    arms[kind + " verified 3 px"] = lambda m=models, k=kind: ctx.match_images_guided(pairs, m, k, 3.0, 0.8, cross)
                    arms[kind + " admit-all"] = lambda m=tile(every), k=kind: ctx.match_images_guided(pairs, m, k, 1e30, 0.8, cross)
                    arms[kind + " fixed model 3 px"] = lambda m=tile(fixed), k=kind: ctx.match_images_guided(pairs, m, k, 3.0, 0.8, cross)
                    found[kind] = int((models["iteration"] >= 0).sum())
                res = timed(arms)
                emit({"case": "guided, " + name, "cross_check": cross, "pairs_with_a_verified_model": found,
                      "matches": {k: int(fn()[0].size) for k, fn in arms.items()}, **res})

    def u8_arms(ctx, cnt):
        import match_u8_ref as U
        n = cnt.size
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        d_kp, d_desc = ctx.result_device_ptrs()
        kp, d8 = ctx.results_u8()
        t8 = torch.from_numpy(d8).cuda()
        nq, nt = int(cnt[0]), int(cnt[1])
        idx = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
        dist = torch.zeros((nq, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def verdict(res):
            f, u = res["f32"], res["u8"]
            overlap = not (u["max_ms"] < f["min_ms"] or f["max_ms"] < u["min_ms"])
            return {"f32_over_u8_medians": round(f["median_ms"] / u["median_ms"], 2), "intervals_overlap": overlap}

        res = timed({"f32": lambda: ctx.knn2_sets(d_desc, off, [(0, 1)], d_kp, idx, dist),
                     "u8": lambda: ctx.knn2_sets_u8(t8, off, [(0, 1)], d_kp, idx, dist)})
        rows = np.random.default_rng(0).choice(nq, size=min(256, nq), replace=False)
        v = kp["has_descriptor"]
        want = U.knn2(d8[off[0]:off[1]][rows], d8[off[1]:off[2]], v[off[0]:off[1]][rows], v[off[1]:off[2]])
        ok = M.same_bits(idx.cpu().numpy()[rows], want[0]) and M.same_bits(dist.cpu().numpy()[rows], want[1])
        emit({"case": "u8 arm, a: frames 1 and 2 of the bench batch, top-2 on device-resident rows", "nq": nq, "nt": nt,
              "spot_check_256_rows_bitwise": bool(ok), **res, **verdict(res)})
        pairs = [(i, i + 1) for i in range(n - 1)]
        for cross in (False, True):
            arms = {"f32": lambda: ctx.match_images(pairs, 0.8, cross), "u8": lambda: ctx.match_images(pairs, 0.8, cross, quantized=True)}
            res = timed(arms)
            emit({"case": f"u8 arm, b: the {len(pairs)} consecutive pairs in one sift_hip_result_match call (ratio 0.8)", "cross_check": cross,
                  "matches": {k: int(fn()[0].size) for k, fn in arms.items()}, **res, **verdict(res)})

    ctx = Context(0)
    # ---- (a) and (b): the bench batch ----
    n = args.frames
    ctx.calculate_batch(synth_batch(n, 1920, 1080), _lib.Params(3, 4, 1.6, K_SQRT2, 0))
    cnt = ctx.counts()
    if args.guided_arm or args.unguided_only or args.u8_arm:
        if args.u8_arm:
            u8_arms(ctx, cnt)
        else:
            guided_arms(ctx, cnt)
        ctx.close()
        if args.out:
            with open(args.out, "a") as f:
                f.write("# tools/match_bench.py --u8-arm: the float matcher alternating with the 8-bit integer matcher (ms on the host around each call)\n"
                        if args.u8_arm else
                        "# tools/match_bench.py --guided-arm: sift_hip_result_match alternating with sift_hip_result_match_guided (ms on the host around each call)\n"
                        if args.guided_arm else "# tools/match_bench.py --unguided-only\n")
                f.write("\n".join(lines) + "\n")
        return
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    kp, desc = ctx.results()
    d_kp, d_desc = ctx.result_device_ptrs()
    tdesc = torch.from_numpy(desc).cuda()
    sets = [tdesc[off[i]:off[i + 1]] for i in range(n)]

    nq, nt = int(cnt[0]), int(cnt[1])
    idx = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    dist = torch.zeros((nq, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res = race(lambda: ctx.knn2_sets(d_desc, off, [(0, 1)], d_kp, idx, dist), lambda: torch_top2(sets[0], sets[1]), 2.0 * nq * nt * 128)
    # spot check: 256 query rows against the host checker, bit for bit
    rows = np.random.default_rng(0).choice(nq, size=min(256, nq), replace=False)
    v = kp["has_descriptor"]
    want = M.knn2(desc[off[0]:off[1]][rows], desc[off[1]:off[2]], v[off[0]:off[1]][rows], v[off[1]:off[2]])
    ok = M.same_bits(idx.cpu().numpy()[rows], want[0]) and M.same_bits(dist.cpu().numpy()[rows], want[1])
    emit({"case": "a: frames 1 and 2 of the bench batch, top-2 on device-resident descriptors", "nq": nq, "nt": nt,
          "spot_check_256_rows_bitwise": bool(ok), **res})

    pairs = [(i, i + 1) for i in range(n - 1)]
    flop = sum(2.0 * int(cnt[a]) * int(cnt[b]) * 128 for a, b in pairs)
    res = race(lambda: ctx.match_images(pairs, 0.8, False), lambda: [torch_top2(sets[a], sets[b]) for a, b in pairs], flop)
    rec, counts = ctx.match_images(pairs, 0.8, False)
    emit({"case": f"b: the {len(pairs)} consecutive pairs of the batch in one sift_hip_result_match call (ratio 0.8), match list to the host",
          "rows": int(sum(cnt[a] for a, _ in pairs)), "matches": int(rec.size), **res})
    res = race(lambda: ctx.match_images(pairs, 0.8, True), lambda: [(torch_top2(sets[a], sets[b]), torch_top2(sets[b], sets[a])) for a, b in pairs], 2 * flop)
    emit({"case": "b with cross-check (both directions)", **res})
    del sets, tdesc

    # ---- (c): the small pair of the tests ----
    big = synth_frame(272, 192, 1)
    ctx.calculate_batch(np.stack([np.ascontiguousarray(big[:, 0:256]), np.ascontiguousarray(big[:, 8:264])]), _lib.Params(3, 3, 1.6, K_SQRT2, 0))
    cnt = ctx.counts()
    kp, desc = ctx.results()
    tdesc = torch.from_numpy(desc).cuda()
    a, b = tdesc[:cnt[0]], tdesc[cnt[0]:]
    res = race(lambda: ctx.match_images([(0, 1)], 0.8, False), lambda: torch_top2(a, b), 2.0 * int(cnt[0]) * int(cnt[1]) * 128)
    emit({"case": "c: 444 x 441, sift_hip_result_match (ratio 0.8), match list to the host", "nq": int(cnt[0]), "nt": int(cnt[1]), **res})
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/match_bench.py: fused GPU matcher against the torch formulation, alternating arms (ms on the host around each call)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
