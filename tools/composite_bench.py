#!/usr/bin/env python3
"""The compositor on ONE box under tools/ab.py's protocol: the arms run ALTERNATELY in one process, at least five alternations,
every arm summarised by the median and the min - max of its samples; a winner between two arms is only named when their
[min, max] intervals do not overlap.

  python3 tools/composite_bench.py [--frames 32] [--width 1920] [--height 1080] [--rounds 5] [--calls 20] [--out profiles/composite_bench.txt]

Frames, models and results are device-resident (torch tensors).  Two workloads:
  stack   the frames under near-identity models (a shift of up to 3 px, up to 0.3 degrees) on one canvas of the frame's size, "mean"
  strip   the frames stepped by a quarter frame (0.2 degrees of rotation) on the canvas that holds them all, "feather"
and three arms:
  path=0       sift_hip_composite_homography, the library chooses per tile and job (staged in LDS, direct or skipped)
  path=1       the same with every tap from global memory
  warp+torch   the parent commit's way: sift_hip_warp_homography of every job onto the full canvas (n canvases and n masks
               written) and a torch reduction of that pile - sum(out * mask) / sum(mask) for "mean"; for "feather" the weight
               image (distance to the border plus one) is warped under every model as n more jobs and the result is
               sum(wgt * out) / sum(wgt) (fill 0 makes the masks unnecessary).  Its sums have no defined order: it is timed,
               not compared - except for "first" on the stack, where it is a gather and is compared bit for bit.
A sample is the host clock around `--calls` calls that end in a device synchronise, per call.  "must move": the bytes an arm
cannot avoid - sources read once, results written once, and for warp+torch the pile written and read back.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def placed(deg, w, h, dx, dy):
    """A rotation by `deg` about the frame's centre, then a shift: canvas lattice -> frame."""
    c, s, cx, cy = math.cos(math.radians(deg)), math.sin(math.radians(deg)), (w - 1) / 2, (h - 1) / 2
    return [c, -s, cx - c * cx + s * cy + dx, s, c, cy - s * cx - c * cy + dy, 0, 0, 1]


def verdict(name, a, b, sa, sb):
    if max(sa) < min(sb) or max(sb) < min(sa):
        return f"  {name:>6} VERDICT: {a if max(sa) < min(sb) else b} is faster than {b if max(sa) < min(sb) else a} (intervals disjoint)"
    return f"  {name:>6} VERDICT: UNRESOLVED between {a} and {b} - the [min, max] intervals overlap"


def main():
    import numpy as np
    import torch
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
        sys.exit("composite_bench.py: no GPU (there is nothing to measure without one)")
    n, w, h = a.frames, a.width, a.height
    ctx = Context(0)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    weight = torch.minimum(torch.minimum(xs, w - 1 - xs), torch.minimum(ys, h - 1 - ys)) + 1.0
    imgs = torch.cat([torch.rand((n, h, w), device="cuda") * 255, weight[None]]).contiguous()   # image n: the weight image
    lines = [f"composite_bench: {n} frames of {w} x {h}, device-resident; {a.rounds} alternations, {a.calls} calls per sample"]
    step = w // 4
    workloads = (
        ("stack", "mean", (h, w), [placed(0.3 * math.sin(k), w, h, 3.0 * math.cos(k), 3.0 * math.sin(2 * k)) for k in range(n)]),
        ("strip", "feather", (h, w + (n - 1) * step), [placed(0.2, w, h, -k * step, 0.0) for k in range(n)]),
    )
    for name, blend, (oh, ow), model_list in workloads:
        models = np.array(model_list, np.float32)
        src = np.arange(n, dtype=np.int32)
        feather = blend == "feather"
        warp_models, warp_src = (np.concatenate([models, models]), np.concatenate([src, np.full(n, n, np.int32)])) if feather else (models, src)
        canvas = torch.empty((1, oh, ow), device="cuda")
        pile = torch.empty((len(warp_models), oh, ow), device="cuda")
        masks = None if feather else torch.empty((n, oh, ow), dtype=torch.uint8, device="cuda")

        def parent():
            ctx.warp_homography(imgs, warp_models, warp_src, (oh, ow), out=pile, mask=masks)
            if feather:
                return (pile[:n] * pile[n:]).sum(0) / pile[n:].sum(0)
            return (pile * masks).sum(0) / masks.sum(0, dtype=torch.float32)

        arms = {
            "path=0": lambda: ctx.composite_homography(imgs, models, None, src, (oh, ow), blend=blend, path=0, out=canvas),
            "path=1": lambda: ctx.composite_homography(imgs, models, None, src, (oh, ow), blend=blend, path=1, out=canvas),
            "warp+torch": parent,
        }
        src_bytes, px = n * w * h * 4, oh * ow
        need = {"path=0": src_bytes + 4 * px, "path=1": src_bytes + 4 * px,
                "warp+torch": (2 if feather else 1) * src_bytes + len(warp_models) * px * 4 * 2 + (0 if feather else n * px * 2) + 4 * px}
        tiles = ctx.composite_homography(imgs, models, None, src, (oh, ow), blend=blend, out=canvas, want_tiles=True)[1]
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
        lines.append(f"{name} ({blend}, canvas {ow} x {oh}): (tile, job) visits staged {tiles[0]}, direct {tiles[1]}, skipped {tiles[2]}")
        for k, s in samples.items():
            med = statistics.median(s)
            lines.append(f"  {name:>6} {k:>10}: median {med:.3f} [{min(s):.3f} - {max(s):.3f}] ms/call, must move {need[k] / 1e6:.1f} MB, "
                         f"{need[k] / (med * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s")
        lines.append(verdict(name, "path=0", "path=1", samples["path=0"], samples["path=1"]))
        best = min(("path=0", "path=1"), key=lambda k: statistics.median(samples[k]))
        lines.append(verdict(name, best, "warp+torch", samples[best], samples["warp+torch"]))
        if name == "stack":   # "first" is a gather: the one blend the parent's way defines bit for bit
            first = ctx.composite_homography(imgs, models, None, src, (oh, ow), fill=-1.0, blend="first", out=canvas)
            ctx.warp_homography(imgs, models, src, (oh, ow), fill=-1.0, out=pile, mask=masks)
            pick = pile.gather(0, masks.to(torch.int64).argmax(0, keepdim=True))   # argmax: the first job whose mask is 1, job 0 where none is
            same = bool((first.view(torch.int32) == pick.view(torch.int32)).all())
            lines.append(f"  {name:>6} first: compositor against warp + gather of the first covering job, bit for bit: {'IDENTICAL' if same else 'DIFFERENT'}")
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
