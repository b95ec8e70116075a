#!/usr/bin/env python3
"""The two-band compositor on ONE box under tools/ab.py's protocol: the arms run ALTERNATELY in one process, at least five
alternations, every arm summarised by the median and the min - max of its samples; a winner between two arms is only named when
their [min, max] intervals do not overlap.

  python3 tools/twoband_bench.py [--frames 32] [--width 1920] [--height 1080] [--rounds 5] [--calls 20] [--out profiles/twoband_bench.txt]

Frames, models and results are device-resident (torch tensors).  The two workloads of tools/composite_bench.py - the stack (near-
identity models on one canvas of the frame's size) and the strip (frames stepped by a quarter frame on the canvas that holds them
all) - each at band sigma 2 (radius 6) and 5 (radius 15), and four arms:
  path=0       sift_hip_composite_twoband, the library chooses per tile and job (constant norm where the window is covered)
  path=1       the same with ln formed from the coverage on every visit
  feather      sift_hip_composite_homography with "feather": what the second band costs
  unfused      sift_hip_warp_homography of every job, and of the weight image under every job's model, onto the full canvas with
               masks; torch.nn.functional.conv2d along x and along y for ls and for ln; bands, weighted low band and the high band
               of the largest weight in torch.  Its planes end at the canvas (zero padding) and its sums have no defined order:
               it is timed, not compared - the largest difference to path=0 away from the canvas border is printed as a check
               that the arms compute the same picture.  It runs a fifth of the calls per sample.
A sample is the host clock around the calls, which end in a device synchronise, per call.  "must move": the bytes an arm cannot
avoid - sources read once, results written once, and for `unfused` the piles and masks written and read back and every pass
reading and writing one plane per job.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from composite_bench import placed, verdict   # noqa: E402


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from sift_amd.sift import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rounds = max(a.rounds, 5)
    if not torch.cuda.is_available():
        sys.exit("twoband_bench.py: no GPU (there is nothing to measure without one)")
    n, w, h = a.frames, a.width, a.height
    ctx = Context(0)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    weight = torch.minimum(torch.minimum(xs, w - 1 - xs), torch.minimum(ys, h - 1 - ys)) + 1.0
    imgs = torch.cat([torch.rand((n, h, w), device="cuda") * 255, weight[None]]).contiguous()   # image n: the weight image
    lines = [f"twoband_bench: {n} frames of {w} x {h}, device-resident; {a.rounds} alternations, {a.calls} calls per sample (unfused: {max(a.calls // 5, 1)})"]
    step = w // 4
    workloads = (
        ("stack", (h, w), [placed(0.3 * math.sin(k), w, h, 3.0 * math.cos(k), 3.0 * math.sin(2 * k)) for k in range(n)]),
        ("strip", (h, w + (n - 1) * step), [placed(0.2, w, h, -k * step, 0.0) for k in range(n)]),
    )
    for name, (oh, ow), model_list in workloads:
        models, src = np.array(model_list, np.float32), np.arange(n, dtype=np.int32)
        warp_models, warp_src = np.concatenate([models, models]), np.concatenate([src, np.full(n, n, np.int32)])
        canvas = torch.empty((1, oh, ow), device="cuda")
        pile = torch.empty((2 * n, oh, ow), device="cuda")
        masks = torch.empty((2 * n, oh, ow), dtype=torch.uint8, device="cuda")
        for sigma in (2.0, 5.0):
            taps = ctx.band_taps(sigma)
            R = taps.size - 1
            kern = torch.from_numpy(np.concatenate([taps[:0:-1], taps])).cuda()

            def blur(x):
                return F.conv2d(F.conv2d(x[:, None], kern.view(1, 1, 1, -1), padding=(0, R)), kern.view(1, 1, -1, 1), padding=(R, 0))[:, 0]

            def unfused():
                ctx.warp_homography(imgs, warp_models, warp_src, (oh, ow), out=pile, mask=masks)   # fill 0: t is 0 where not covered
                t, wgt, m = pile[:n], pile[n:], masks[:n]
                low = torch.where(m > 0, blur(t) / blur(m.float()), 0.0)
                high = (t - low).gather(0, wgt.argmax(0, keepdim=True))[0]
                return (wgt * low).sum(0) / wgt.sum(0) + high

            arms = {
                "path=0": lambda: ctx.composite_twoband(imgs, models, None, src, (oh, ow), taps=taps, path=0, out=canvas),
                "path=1": lambda: ctx.composite_twoband(imgs, models, None, src, (oh, ow), taps=taps, path=1, out=canvas),
                "feather": lambda: ctx.composite_homography(imgs, models, None, src, (oh, ow), blend="feather", out=canvas),
                "unfused": unfused,
            }
            calls = {k: (max(a.calls // 5, 1) if k == "unfused" else a.calls) for k in arms}
            src_bytes, px = n * w * h * 4, oh * ow
            fused = src_bytes + 4 * px
            need = {"path=0": fused, "path=1": fused, "feather": fused,
                    "unfused": 2 * src_bytes + 2 * (2 * n * px * 4 + 2 * n * px) + 4 * 2 * n * px * 4 + 4 * px}
            tiles = ctx.composite_twoband(imgs, models, None, src, (oh, ow), taps=taps, out=canvas, want_tiles=True)[1]
            samples = {k: [] for k in arms}
            for fn in arms.values():   # warm every arm
                fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls[k]):
                        fn()
                    torch.cuda.synchronize()
                    samples[k].append((time.perf_counter() - t0) * 1e3 / calls[k])
            tag = f"{name} s={sigma:g}"
            lines.append(f"{tag} (radius {R}, canvas {ow} x {oh}): (tile, job) visits general {tiles[0]}, constant-norm {tiles[1]}, skipped {tiles[2]}")
            for k, s in samples.items():
                med = statistics.median(s)
                lines.append(f"  {tag:>11} {k:>8}: median {med:.3f} [{min(s):.3f} - {max(s):.3f}] ms/call, must move {need[k] / 1e6:.1f} MB, "
                             f"{need[k] / (med * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s")
            lines.append(verdict(tag, "path=0", "path=1", samples["path=0"], samples["path=1"]))
            best = min(("path=0", "path=1"), key=lambda k: statistics.median(samples[k]))
            lines.append(verdict(tag, best, "feather", samples[best], samples["feather"]))
            lines.append(verdict(tag, best, "unfused", samples[best], samples["unfused"]))
            if name == "stack":
                arms["path=0"]()
                diff = (unfused() - canvas[0])[R:oh - R, R:ow - R].abs()   # the frames are independent noise: where two weights nearly
                lines.append(f"  {tag:>11} check: |unfused - path=0| away from the canvas border: median {diff.median().item():.3g}, "   # tie, the arms' high bands differ
                             f"above 0.01 on a share of {(diff > 0.01).float().mean().item():.2g} of the pixels (values 0 .. 255)")
        del pile, masks, canvas
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
