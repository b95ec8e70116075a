"""Geometric verification on the GPU, measured (bench.py measures extraction and is left alone).

Cases, all at --iterations hypotheses per set (2048) and a 3 px threshold: (a) the match list of frames 1 and 2 of the bench
batch (ratio 0.8), its coordinates resident on the device, through sift_hip_ransac_homography; (b) the 31 consecutive pairs of
the 32-frame batch through ONE sift_hip_result_verify call (matching + coordinates + RANSAC, records, flags and models to the
host), beside sift_hip_result_match alone and the RANSAC alone on the same lists; (c) one synthetic list of 20 000 rows, where
the scoring kernel and not the launches sets the time.  Comparators on the same rows: the torch formulation on the same GPU -
SCORING ONLY, given a table of models: batched H @ pts, the division-free comparison, sum, argmax (no sampling, no solve: that
favours it) - alternating with the library's arm in the same run, and the host loop (hostmath_ransac_homography) on one core.
The models and flags of every case are compared bit for bit with the host loop.

Timing: a warm-up, then --reps repetitions of each arm in turn; median and min - max of the host time around each call (the
library's calls return when the result is in place; the torch arm ends in a synchronize).  predicates/s = sets' rows x
iterations / time (invalid hypotheses are not scored, so the work done is smaller: "valid_share").

The refine arm (--refine-arm) runs the RANSAC-alone cases (a), (b) and (c) with `refine` 0 and `refine` 2 alternating in one run -
the difference of the medians is what the refinement stage (one more launch, ransac_refine_kernel) adds to a call - compares the
refined models and flags bit for bit with the host loop (hostmath_ransac_homography_refined), and records the corner error of
the minimal-sample and the refined model on the synthetic case of tests/test_refine_host.py (600 rows, 60 % outliers, 0.5 px
noise, 512 hypotheses, seeds 0 .. 19, `refine` 8).  It APPENDS its lines to --out.

The fundamental arm (--fundamental-arm) runs the same three RANSAC-alone cases through sift_hip_ransac_fundamental (seven-point
samples, 3 x iterations hypothesis slots per set), alternating with sift_hip_ransac_homography at the same iterations on the same
GPU, beside the host loop (hostmath_ransac_fundamental) on one core; models and flags are compared bit for bit with that loop.
The rows are those of the homography cases: the question is what the call costs, not whether the scenes determine F.  It
APPENDS its lines to --out.

    python tools/ransac_bench.py [--reps 20] [--frames 32] [--out profiles/ransac_bench.txt]
    python tools/ransac_bench.py --refine-arm [--reps 20] [--out profiles/ransac_bench.txt]
    python tools/ransac_bench.py --fundamental-arm [--reps 20] [--out profiles/ransac_bench.txt]
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
    ap.add_argument("--iterations", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--refine-arm", action="store_true", help="only the refine arm: refine 0 against refine 2, appended to --out")
    ap.add_argument("--fundamental-arm", action="store_true",
                    help="only the fundamental arm: sift_hip_ransac_fundamental against sift_hip_ransac_homography, appended to --out")
    args = ap.parse_args()

    import torch
    import ransac_ref as R
    import refine_ref as F
    import fund_ref
    from sift_amd import _lib
    from sift_amd.sift import Context, K_SQRT2
    from sift_amd.synthetic import synth_batch

    lines = []
    its, thr = args.iterations, 3.0

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    def race(fused, comparator):
        for _ in range(args.warmup):
            fused()
            comparator()
        torch.cuda.synchronize()
        f_ms, t_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fused()
            f_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            comparator()
            torch.cuda.synchronize()
            t_ms.append((time.perf_counter() - t0) * 1e3)
        return stats(f_ms), stats(t_ms)

    def torch_score(tpts, toff, hs):
        """Per set: scores of `hs` [I, 3, 3] over the set's rows, and the argmax.  float32 throughout."""
        out = []
        for s in range(len(toff) - 1):
            p = tpts[toff[s]:toff[s + 1]]
            if p.shape[0] == 0:
                continue
            q = torch.cat([p[:, :2], torch.ones_like(p[:, :1])], dim=1)
            xyw = hs @ q.T                                               # [I, 3, m]
            ex, ey = xyw[:, 0] - p[:, 2] * xyw[:, 2], xyw[:, 1] - p[:, 3] * xyw[:, 2]
            inl = (xyw[:, 2] > 0) & (ex * ex + ey * ey <= (thr * thr) * xyw[:, 2] * xyw[:, 2])
            out.append(torch.argmax(inl.sum(dim=1)))
        return out

    def coords(kp, row0, idx):
        k = kp[row0 + idx]
        return np.stack([k["x"].astype(np.int64) << k["octave"], k["y"].astype(np.int64) << k["octave"]], axis=1).astype(np.float32)

    def case(name, ctx, pts, off, extra):
        """RANSAC alone on rows resident on the device, against the torch scoring and the host loop."""
        n_sets = off.size - 1
        dpts = torch.from_numpy(pts).cuda()
        dm = torch.zeros((n_sets, 12), dtype=torch.int32, device="cuda")
        df = torch.zeros((max(pts.shape[0], 1),), dtype=torch.uint8, device="cuda")
        hs = (torch.eye(3, device="cuda")[None] + 1e-4 * torch.randn((its, 3, 3), device="cuda")).contiguous()
        toff = off.tolist()
        torch.cuda.synchronize()
        f, t = race(lambda: ctx.ransac_homography(dpts, off, its, thr, 0, models_out=dm, inlier_out=df), lambda: torch_score(dpts, toff, hs))
        host = timed(lambda: R.ransac(pts, off, its, thr, 0), 3)
        want = R.ransac(pts, off, its, thr, 0)
        ok = dm.cpu().numpy().tobytes() == want[0].tobytes() and df.cpu().numpy()[:pts.shape[0]].tobytes() == want[1].tobytes()
        pred = float(pts.shape[0]) * its
        emit({"case": name, "sets": int(n_sets), "rows": int(pts.shape[0]), "iterations": its, "valid_share": round(float((want[2] >= 0).mean()), 3),
              "inliers": want[0]["inliers"].tolist()[:4], "bitwise_equal_to_host_loop": bool(ok), "gpu": f, "torch_scoring_only": t,
              "host_loop_one_core": host, "gpu_gpred_per_s": round(pred / (f["median_ms"] * 1e-3) / 1e9, 2),
              "speedup_vs_torch": round(t["median_ms"] / f["median_ms"], 2), "speedup_vs_host_loop": round(host["median_ms"] / f["median_ms"], 1),
              **extra})

    def refine_case(name, ctx, pts, off, rounds=2):
        """The same call with refine 0 and with refine `rounds`, alternating; rows and results resident on the device."""
        n_sets = off.size - 1
        dpts = torch.from_numpy(pts).cuda()
        dm = torch.zeros((n_sets, 12), dtype=torch.int32, device="cuda")
        df = torch.zeros((max(pts.shape[0], 1),), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plain, fine = race(lambda: ctx.ransac_homography(dpts, off, its, thr, 0, models_out=dm, inlier_out=df),
                           lambda: ctx.ransac_homography(dpts, off, its, thr, 0, models_out=dm, inlier_out=df, refine=rounds))
        want = F.ransac(pts, off, its, thr, 0, refine=rounds)
        base = R.ransac(pts, off, its, thr, 0)
        ok = dm.cpu().numpy().tobytes() == want[0].tobytes() and df.cpu().numpy()[:pts.shape[0]].tobytes() == want[1].tobytes()
        emit({"case": "refine arm, " + name, "sets": int(n_sets), "rows": int(pts.shape[0]), "iterations": its, "refine": rounds,
              "bitwise_equal_to_host_loop": bool(ok), "refine_0": plain, f"refine_{rounds}": fine,
              "added_ms_median": round(fine["median_ms"] - plain["median_ms"], 4), "rounds_accepted": want[0]["refined"].tolist()[:8],
              "inliers_minimal": base[0]["inliers"].tolist()[:8], "inliers_refined": want[0]["inliers"].tolist()[:8]})

    def fund_case(name, ctx, pts, off):
        """sift_hip_ransac_fundamental and sift_hip_ransac_homography at the same iterations, alternating; rows and results on the device."""
        n_sets = off.size - 1
        dpts = torch.from_numpy(pts).cuda()
        dm = torch.zeros((n_sets, 12), dtype=torch.int32, device="cuda")
        dh = torch.zeros((n_sets, 12), dtype=torch.int32, device="cuda")
        df = torch.zeros((max(pts.shape[0], 1),), dtype=torch.uint8, device="cuda")
        dg = torch.zeros((max(pts.shape[0], 1),), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fund, homo = race(lambda: ctx.ransac_fundamental(dpts, off, its, thr, 0, models_out=dm, inlier_out=df),
                          lambda: ctx.ransac_homography(dpts, off, its, thr, 0, models_out=dh, inlier_out=dg))
        host = timed(lambda: fund_ref.ransac(pts, off, its, thr, 0), 3)
        want = fund_ref.ransac(pts, off, its, thr, 0)
        ok = dm.cpu().numpy().tobytes() == want[0].tobytes() and df.cpu().numpy()[:pts.shape[0]].tobytes() == want[1].tobytes()
        emit({"case": "fundamental arm, " + name, "sets": int(n_sets), "rows": int(pts.shape[0]), "iterations": its, "slots_per_set": 3 * its,
              "valid_share": round(float((want[2] >= 0).mean()), 3), "inliers": want[0]["inliers"].tolist()[:4],
              "bitwise_equal_to_host_loop": bool(ok), "fundamental": fund, "homography_same_iterations": homo, "host_loop_one_core": host,
              "ratio_to_homography": round(fund["median_ms"] / homo["median_ms"], 2),
              "speedup_vs_host_loop": round(host["median_ms"] / fund["median_ms"], 1)})

    def finish(mode, header):
        if args.out:
            with open(args.out, mode) as f:
                for h in header:
                    f.write(h)
                f.write("\n".join(lines) + "\n")

    ctx = Context(0)
    n = args.frames
    ctx.calculate_batch(synth_batch(n, 1920, 1080), _lib.Params(3, 4, 1.6, K_SQRT2, 0))
    cnt = ctx.counts()
    row0 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    kp, _ = ctx.results()

    # ---- (a): two 1080p frames' match list ----
    rec, counts = ctx.match_images([(0, 1)], 0.8, False)
    pts = np.concatenate([coords(kp, row0[0], rec["query"]), coords(kp, row0[1], rec["train"])], axis=1)
    if args.fundamental_arm:
        fund_case("a: match list of frames 1 and 2 of the bench batch", ctx, pts, np.array([0, pts.shape[0]], np.int64))
        pairs = [(i, i + 1) for i in range(n - 1)]
        rec, counts = ctx.match_images(pairs, 0.8, False)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.zeros((rec.size, 4), np.float32)
        for p, (a, b) in enumerate(pairs):
            r = rec[off[p]:off[p + 1]]
            pts[off[p]:off[p + 1]] = np.concatenate([coords(kp, row0[a], r["query"]), coords(kp, row0[b], r["train"])], axis=1)
        fund_case(f"b: the {len(pairs)} lists of consecutive pairs as the sets of one call", ctx, pts, off)
        rows, _ = R.projective_rows(np.random.default_rng(0), 20000)
        fund_case("c: 20 000 synthetic correspondences (60 % outliers)", ctx, rows, np.array([0, 20000], np.int64))
        ctx.close()
        finish("a", [])
        return
    if args.refine_arm:
        refine_case("a: match list of frames 1 and 2 of the bench batch", ctx, pts, np.array([0, pts.shape[0]], np.int64))
        pairs = [(i, i + 1) for i in range(n - 1)]
        rec, counts = ctx.match_images(pairs, 0.8, False)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = np.zeros((rec.size, 4), np.float32)
        for p, (a, b) in enumerate(pairs):
            r = rec[off[p]:off[p + 1]]
            pts[off[p]:off[p + 1]] = np.concatenate([coords(kp, row0[a], r["query"]), coords(kp, row0[b], r["train"])], axis=1)
        refine_case(f"b: the {len(pairs)} lists of consecutive pairs as the sets of one call", ctx, pts, off)
        rows, _ = R.projective_rows(np.random.default_rng(0), 20000)
        refine_case("c: 20 000 synthetic correspondences (60 % outliers)", ctx, rows, np.array([0, 20000], np.int64))
        e0, e1, ok = [], [], True
        for seed in range(20):
            rows, _ = R.projective_rows(np.random.default_rng(seed), 600, outliers=0.6, noise=0.5)
            base = ctx.ransac_homography(rows, None, 512, thr, seed)[0][0]
            got = ctx.ransac_homography(rows, None, 512, thr, seed, refine=8)
            want = F.ransac(rows, None, 512, thr, seed, refine=8)
            ok = ok and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            e0.append(F.corner_error(base["h"]))
            e1.append(F.corner_error(got[0][0]["h"]))
        emit({"case": "refine arm, corner error on the 1000 px square: 600 rows, 60 % outliers, 0.5 px noise, 512 hypotheses, seeds 0 .. 19, refine 8",
              "bitwise_equal_to_host_loop": bool(ok), "minimal_px": {"min": round(min(e0), 3), "median": round(statistics.median(e0), 3), "max": round(max(e0), 3)},
              "refined_px": {"min": round(min(e1), 3), "median": round(statistics.median(e1), 3), "max": round(max(e1), 3)},
              "seeds_improved": int(sum(b < a for a, b in zip(e0, e1)))})
        ctx.close()
        finish("a", [])
        return
    case("a: match list of frames 1 and 2 of the bench batch (ratio 0.8), rows on the device, sift_hip_ransac_homography", ctx, pts,
         np.array([0, pts.shape[0]], np.int64), {"keypoints": [int(cnt[0]), int(cnt[1])]})

    # ---- (b): 31 pairs in one call ----
    pairs = [(i, i + 1) for i in range(n - 1)]
    for _ in range(args.warmup):
        ctx.verify_images(pairs, 0.8, False, its, thr, 0)
        ctx.match_images(pairs, 0.8, False)
    v_ms, m_ms = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ctx.verify_images(pairs, 0.8, False, its, thr, 0)
        v_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.match_images(pairs, 0.8, False)
        m_ms.append((time.perf_counter() - t0) * 1e3)
    rec, counts, models, flags = ctx.verify_images(pairs, 0.8, False, its, thr, 0)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.zeros((rec.size, 4), np.float32)
    for p, (a, b) in enumerate(pairs):
        r = rec[off[p]:off[p + 1]]
        pts[off[p]:off[p + 1]] = np.concatenate([coords(kp, row0[a], r["query"]), coords(kp, row0[b], r["train"])], axis=1)
    want = R.ransac(pts, off, its, thr, 0)
    ok = models.astype(R.MODEL_DTYPE).tobytes() == want[0].tobytes() and flags.tobytes() == want[1].tobytes()
    emit({"case": f"b: the {len(pairs)} consecutive pairs of the batch in one sift_hip_result_verify call (ratio 0.8), records, flags and models to the host",
          "matches": int(rec.size), "iterations": its, "bitwise_equal_to_host_loop": bool(ok), "result_verify": stats(v_ms),
          "result_match_alone": stats(m_ms), "difference_of_medians_ms": round(statistics.median(v_ms) - statistics.median(m_ms), 4)})
    case("b, the RANSAC alone: the same 31 lists as the sets of one sift_hip_ransac_homography call, rows on the device", ctx, pts, off, {})

    # ---- (c): one long list ----
    rows, _ = R.projective_rows(np.random.default_rng(0), 20000)
    case("c: 20 000 synthetic correspondences (60 % outliers), rows on the device", ctx, rows, np.array([0, 20000], np.int64), {})
    ctx.close()
    finish("w", ["# tools/ransac_bench.py: GPU RANSAC homography against the torch scoring formulation (same GPU, alternating) and the host loop (ms on the host around each call)\n",
                 "# solver: largest deviation of ransac_homography4 from numpy's float64 8x8 solution over tests/test_ransac_host.py's samples, both scaled by their largest entry: 1.16e-08\n"])


if __name__ == "__main__":
    main()
