#!/usr/bin/env python3
"""The overlap statistics on ONE box under tools/ab.py's protocol: the arms run ALTERNATELY in one process, at least five
alternations, every arm summarised by the median and the min - max of its samples; a winner between two arms is only named when
their [min, max] intervals do not overlap.

  python3 tools/overlap_bench.py [--frames 32] [--width 1920] [--height 1080] [--rounds 5] [--calls 10] [--out profiles/overlap_bench.txt]

Frames, models and results are device-resident (torch tensors).  The two workloads of tools/composite_bench.py:
  stack   the frames under near-identity models (a shift of up to 3 px, up to 0.3 degrees) on one canvas of the frame's size
  strip   the frames stepped by a quarter frame (0.2 degrees of rotation) on the canvas that holds them all
and three arms:
  path=0       sift_hip_overlap_stats with gains, a 64 x 64 region's 16 chunks share one flush
  path=1       the same with every chunk flushed by itself (16 x the atomics; the difference prices a flush)
  warp+torch   the parent commit's way: sift_hip_warp_homography of every job onto the full canvas (n canvases and n masks
               written), the quantiser in torch and four matrix products of the masked pile, in float32: its sums are not
               exact and have no defined order, so it is timed, not compared
A sample is the host clock around `--calls` calls that end in a device synchronise, per call.  "must move": the bytes an arm
cannot avoid - sources read once, the statistics written, and for warp+torch the pile and the masks written and read back.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.composite_bench import placed, verdict   # noqa: E402


def main():
    import numpy as np
    import torch
    from sift_amd.sift import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rounds = max(a.rounds, 5)
    if not torch.cuda.is_available():
        sys.exit("overlap_bench.py: no GPU (there is nothing to measure without one)")
    n, w, h = a.frames, a.width, a.height
    ctx = Context(0)
    imgs = (torch.rand((n, h, w), device="cuda") * 255).contiguous()
    lines = [f"overlap_bench: {n} frames of {w} x {h}, device-resident; {a.rounds} alternations, {a.calls} calls per sample"]
    step = w // 4
    workloads = (
        ("stack", (h, w), [placed(0.3 * math.sin(k), w, h, 3.0 * math.cos(k), 3.0 * math.sin(2 * k)) for k in range(n)]),
        ("strip", (h, w + (n - 1) * step), [placed(0.2, w, h, -k * step, 0.0) for k in range(n)]),
    )
    for name, (oh, ow), model_list in workloads:
        models = np.array(model_list, np.float32)
        src = np.arange(n, dtype=np.int32)
        stats = torch.zeros((1, 4, 32, 32), dtype=torch.int64, device="cuda")
        gains = torch.ones(n, dtype=torch.float32, device="cuda")
        pile = torch.empty((n, oh, ow), device="cuda")
        masks = torch.empty((n, oh, ow), dtype=torch.uint8, device="cuda")

        def parent():
            ctx.warp_homography(imgs, models, src, (oh, ow), out=pile, mask=masks)
            c = masks.view(n, -1).to(torch.float32)
            q = torch.clamp(torch.floor(pile.view(n, -1) + 0.5), 0, 255) * c
            return c @ c.T, q @ c.T, (q * q) @ c.T, q @ q.T

        arms = {
            "path=0": lambda: ctx.overlap_stats(imgs, models, None, src, (oh, ow), gains=gains, path=0, stats=stats),
            "path=1": lambda: ctx.overlap_stats(imgs, models, None, src, (oh, ow), gains=gains, path=1, stats=stats),
            "warp+torch": parent,
        }
        src_bytes, px = n * w * h * 4, oh * ow
        need = {"path=0": src_bytes + 4 * 32 * 32 * 8, "path=1": src_bytes + 4 * 32 * 32 * 8, "warp+torch": src_bytes + n * px * (4 + 1) * 2}
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
        pairs = int((stats[0, 0] > 0).sum())
        regions = ((ow + 63) // 64) * ((oh + 63) // 64)
        lines.append(f"{name} (canvas {ow} x {oh}): {regions} regions of 64 x 64, {pairs} of {n * n} ordered pairs overlap")
        for k, s in samples.items():
            med = statistics.median(s)
            lines.append(f"  {name:>6} {k:>10}: median {med:.3f} [{min(s):.3f} - {max(s):.3f}] ms/call, must move {need[k] / 1e6:.1f} MB, "
                         f"{need[k] / (med * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s")
        lines.append(verdict(name, "path=0", "path=1", samples["path=0"], samples["path=1"]))
        best = min(("path=0", "path=1"), key=lambda k: statistics.median(samples[k]))
        lines.append(verdict(name, best, "warp+torch", samples[best], samples["warp+torch"]))
        if name == "stack":   # every pair overlaps in every region: the flush at its fullest
            flushes = regions * ((min(oh, 64) + 3) // 4)
            lines.append(f"  {name:>6} atomics: at most {regions * 4 * pairs} 64-bit adds a call on {4 * pairs} addresses with path=0 (one flush a region), "
                         f"at most {flushes * 4 * pairs} with path=1 ({flushes} flushes); the medians differ by "
                         f"{statistics.median(samples['path=1']) - statistics.median(samples['path=0']):.3f} ms for the {flushes - regions} extra flushes")
        del pile, masks
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
