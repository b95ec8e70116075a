#!/usr/bin/env python3
"""The homography warp on ONE box under tools/ab.py's protocol: the arms run ALTERNATELY, at least five alternations, every arm
summarised by the median and the min - max of its samples; a winner between two arms is only named when their [min, max]
intervals do not overlap.

  python3 tools/warp_bench.py [--jobs 32] [--width 1920] [--height 1080] [--rounds 5] [--calls 10] [--out profiles/warp_bench.txt]

Jobs, images and results are device-resident (torch tensors).  For each of three models - near-identity (a 3 px shift with 0.5
degrees of rotation), a 30 degree and a 90 degree rotation about the centre - the arms are
  path=0       sift_hip_warp_homography, the library chooses per tile (staged in LDS or direct)
  path=1       every tile reads its taps from global memory
  grid_sample  torch.nn.functional.grid_sample (bilinear, zeros, align_corners=True) with its grid built outside the timed region
  grid+sample  the same with the grid built inside it (what a caller pays who holds a model, not a grid)
A sample is the host clock around `--calls` calls that end in a device synchronise, per call.  "of 8 TB/s": the bytes the warp
must move - every source image read once, every output pixel written once, 4 bytes each - over the time, as a share of the peak.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rotation(deg, w, h, shift=0.0):
    c, s, cx, cy = math.cos(math.radians(deg)), math.sin(math.radians(deg)), (w - 1) / 2, (h - 1) / 2
    return [c, -s, cx - c * cx + s * cy + shift, s, c, cy - s * cx - c * cy + shift, 0, 0, 1]


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from sift_amd.sift import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rounds = max(a.rounds, 5)
    if not torch.cuda.is_available():
        sys.exit("warp_bench.py: no GPU (there is nothing to measure without one)")
    n, w, h = a.jobs, a.width, a.height
    ctx = Context(0)
    imgs = torch.rand((n, h, w), device="cuda") * 255
    out = torch.empty((n, h, w), device="cuda")
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    need = 2.0 * n * w * h * 4
    lines = [f"warp_bench: {n} jobs of {w} x {h}, device-resident; {a.rounds} alternations, {a.calls} calls per sample; bytes needed per call {need / 1e6:.1f} MB"]

    def grid_of(m):
        W = m[6] * xs + m[7] * ys + m[8]
        u, v = (m[0] * xs + m[1] * ys + m[2]) / W, (m[3] * xs + m[4] * ys + m[5]) / W
        return torch.stack([u * (2.0 / (w - 1)) - 1.0, v * (2.0 / (h - 1)) - 1.0], dim=-1)[None].expand(n, h, w, 2)

    for name, model in (("near-identity", rotation(0.5, w, h, 3.0)), ("rot30", rotation(30.0, w, h)), ("rot90", rotation(90.0, w, h))):
        models = np.tile(np.array(model, np.float32), (n, 1))
        grid = grid_of(model).contiguous()
        arms = {
            "path=0": lambda: ctx.warp_homography(imgs, models, out=out, path=0),
            "path=1": lambda: ctx.warp_homography(imgs, models, out=out, path=1),
            "grid_sample": lambda: F.grid_sample(imgs[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True),
            "grid+sample": lambda: F.grid_sample(imgs[:, None], grid_of(model), mode="bilinear", padding_mode="zeros", align_corners=True),
        }
        tiles = ctx.warp_homography(imgs, models, out=out, want_tiles=True)[1]
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
        lines.append(f"{name}: tiles staged {tiles[0]}, direct {tiles[1]}")
        for k, s in samples.items():
            med = statistics.median(s)
            lines.append(f"  {name:>13} {k:>11}: median {med:.3f} [{min(s):.3f} - {max(s):.3f}] ms/call, {need / (med * 1e-3) / 8e12 * 100:.1f} % of 8 TB/s")
        (s0, s1) = samples["path=0"], samples["path=1"]
        if max(s0) < min(s1) or max(s1) < min(s0):
            lines.append(f"  {name:>13} VERDICT: {'path=0' if max(s0) < min(s1) else 'path=1'} is faster (intervals disjoint)")
        else:
            lines.append(f"  {name:>13} VERDICT: UNRESOLVED between path=0 and path=1 - the [min, max] intervals overlap")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
