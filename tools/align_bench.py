#!/usr/bin/env python3
"""The direct alignment on ONE box under tools/ab.py's protocol: the arms run ALTERNATELY, at least five alternations, every arm
summarised by the median and the min - max of its samples; a winner between two arms is only named when their [min, max]
intervals do not overlap.

  python3 tools/align_bench.py [--frames 32] [--width 1920] [--height 1080] [--align 4] [--rounds 5] [--calls 5] [--out profiles/align_bench.txt]

The frames are consecutive crops of one synthetic scene (sift_amd.synthetic.synth_frame, the benchmark's generator), each 1.5
pixels further along than the one before and 3 % brighter; pair k is (k, k + 1), and its start model is the true shift less 0.6 pixel.
Frames, models and results are device-resident (torch tensors).  The arms:
  path=0    sift_hip_align_homography, 16 pixels a lane with the ballot skip
  path=1    the masked kernel
  unfused   what a caller had before: per round Context.warp_homography, central differences of the warped frame in torch, a
            materialised [pixels x 10] Jacobian, J^T J, J^T r and torch.linalg.solve (float32; affine-plus-perspective columns in raw
            pixels, no acceptance test: it is only timed, its result is not used)
Why not the benchmark's own 32 frames: synth_frame(w, h, seed) draws an independent noise field per seed, so consecutive frames of
that batch share no scene and no model registers them.  After the timing: rms0 -> rms of the call, and Context.overlap_zncc of
every pair under its start and under its aligned model.
A sample is the host clock around `--calls` calls that end in a device synchronise, per call.  "of 8 TB/s": the bytes the passes
must move - both frames of every pair read once per pass, 4 bytes a pixel - over the time, as a share of the peak.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from sift_amd import _lib
    from sift_amd.sift import Context
    from sift_amd.synthetic import synth_frame
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--align", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rounds = max(a.rounds, 5)
    if not torch.cuda.is_available():
        sys.exit("align_bench.py: no GPU (there is nothing to measure without one)")
    n, w, h, step = a.frames, a.width, a.height, 1.5
    scene = torch.from_numpy(synth_frame(w + 64, h, 1).astype(np.float32)).cuda()
    xs = torch.arange(w, device="cuda", dtype=torch.float32)
    frames = []
    for k in range(n):   # a crop at the fractional offset k * step: linear interpolation along x, exact enough for a timing workload
        x0 = xs + k * step
        i0, f = x0.floor().long(), x0 - x0.floor()
        frames.append((scene[:, i0] * (1 - f) + scene[:, i0 + 1] * f) * (1.03 ** k))
    imgs = torch.stack(frames).contiguous()
    pairs = [(k, k + 1) for k in range(n - 1)]
    start = np.zeros(n - 1, _lib.HOMOGRAPHY_DTYPE)
    start["h"] = np.array([1, 0, -step + 0.6, 0, 1, 0, 0, 0, 1], np.float32)
    d_start = torch.from_numpy(start.view(np.uint8)).cuda()
    d_models, d_out = d_start.clone(), torch.zeros((n - 1) * _lib.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx = Context(0)
    need = 2.0 * (n - 1) * w * h * 4 * (a.align + 1)
    lines = [f"align_bench: {n - 1} pairs of {w} x {h}, device-resident, rounds = {a.align}; {a.rounds} alternations, {a.calls} calls per sample; "
             f"bytes needed per call {need / 1e6:.1f} MB"]

    def library(path):
        d_models.copy_(d_start)
        ctx.align_homography(imgs, pairs, d_models, a.align, path=path, out=d_out)

    ys, xg = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), xs, indexing="ij")
    src = [t for _, t in pairs]

    def unfused():
        H = torch.from_numpy(np.ascontiguousarray(start["h"])).cuda()
        for _ in range(a.align):
            warped, mask = ctx.warp_homography(imgs, H, src, mask=torch.empty((n - 1, h, w), dtype=torch.uint8, device="cuda"),
                                               out=torch.empty((n - 1, h, w), device="cuda"), shape=(n, h, w))
            gx = torch.zeros_like(warped)
            gy = torch.zeros_like(warped)
            gx[:, :, 1:-1] = 0.5 * (warped[:, :, 2:] - warped[:, :, :-2])
            gy[:, 1:-1] = 0.5 * (warped[:, 2:] - warped[:, :-2])
            m = mask.float()
            cols = [gx * xg, gx * ys, gx, gy * xg, gy * ys, gy, -(gx * xg + gy * ys) * xg, -(gx * xg + gy * ys) * ys, warped, torch.ones_like(warped)]
            J = torch.stack([c * m for c in cols], dim=-1).reshape(n - 1, h * w, 10)
            r = ((imgs[:n - 1] - warped) * m).reshape(n - 1, h * w, 1)
            JtJ = J.transpose(1, 2) @ J + 1e-3 * torch.eye(10, device="cuda")
            d = torch.linalg.solve(JtJ, J.transpose(1, 2) @ r)[:, :, 0]
            H = H.clone()
            H[:, :8] += d[:, :8]

    arms = {"path=0": lambda: library(0), "path=1": lambda: library(1), "unfused": unfused}
    samples = {k: [] for k in arms}
    for fn in arms.values():   # warm every arm
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) * 1e3 / a.calls)
    for k, s in samples.items():
        med = statistics.median(s)
        lines.append(f"  {k:>8}: median {med:.3f} [{min(s):.3f} - {max(s):.3f}] ms/call, {need / (med * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s")
    s0, s1 = samples["path=0"], samples["path=1"]
    if max(s0) < min(s1) or max(s1) < min(s0):
        lines.append(f"  VERDICT: {'path=0' if max(s0) < min(s1) else 'path=1'} is faster (intervals disjoint)")
    else:
        lines.append("  VERDICT: UNRESOLVED between path=0 and path=1 - the [min, max] intervals overlap")
    library(0)
    res = d_out.cpu().numpy().view(_lib.ALIGNMENT_DTYPE)
    lines.append(f"  rms0 -> rms over the pairs: median {np.median(res['rms0']):.3f} -> {np.median(res['rms']):.3f}, worst {res['rms0'].max():.3f} -> "
                 f"{res['rms'].max():.3f}; rounds accepted {res['rounds'].min()} .. {res['rounds'].max()}; status counts "
                 f"{np.bincount(res['status'], minlength=6).tolist()}; pixels median {int(np.median(res['pixels']))}")
    # the library's own measure of registration: the ZNCC of frame q and of frame t under the model, over the pixels
    # both cover, one canvas per pair; scale brings the brightest frame's values into 0 .. 255
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    offsets, both = np.arange(0, 2 * n - 1, 2), np.array(pairs, np.int32).reshape(-1)

    def zncc(h9):
        jobs = np.stack([ident if k % 2 == 0 else h9[k // 2] for k in range(2 * (n - 1))])
        stats = ctx.overlap_stats(imgs, jobs, offsets, both, scale=1.0 / 1.03 ** (n - 1), shape=(n, h, w))
        return np.array([ctx.overlap_zncc(st, 2)[0, 1] for st in stats])

    z0, z1 = zncc(start["h"]), zncc(res["h"])
    lines.append(f"  overlap_zncc under the start -> the aligned models: median {np.median(z0):.5f} -> {np.median(z1):.5f}, worst {z0.min():.5f} -> "
                 f"{z1.min():.5f}; pairs whose ZNCC fell: {int((z1 < z0).sum())} of {n - 1}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
