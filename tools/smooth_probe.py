#!/usr/bin/env python3
"""The smooth splat (raster_smooth_ / raster_pullback_smooth_) on one MI355X, fp32.

    python tools/smooth_probe.py [--reps 9] [--out profiles/smooth_probe.txt]

For 128^3, 256^3 and 512^2 (3-D points), P from 1e4 to 1e7 and B in {1, 16}, for a uniform cloud as generated
("random") and after dpr_amd.sort_points ("hilbert"): the forward on DPR_ALGO_ATOMIC and on DPR_ALGO_TILED, the
atomic pullback, and the linear `raster_` (AUTO) of the same shape as a bar.  Inputs are resident on the device,
workspaces allocated once.  Times: median over `--reps` of HIP events around one call (ms) after a warm-up call of
every variant; the variants of a shape are timed in turn within each repetition, so that drift hits them alike.  The
last column is the spread (max - min) / median of the two smooth forwards over the repetitions, the larger of the two."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

GRIDS = [("128^3", (128, 128, 128)), ("256^3", (256, 256, 256)), ("512^2", (512, 512))]
POINTS = [10_000, 30_000, 100_000, 300_000, 1_000_000, 10_000_000]
BATCHES = [1, 16]


def timed_in_turn(fns, reps):
    """{name: list of ms}: one warm-up call each, then `reps` rounds of every variant in turn."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return ts


def ws(n, dev):
    return torch.empty(max(n, 256), dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_probe.txt"))
    ap.add_argument("--grids", default=",".join(g[0] for g in GRIDS))
    ap.add_argument("--max-points", type=int, default=POINTS[-1])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/smooth_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; points "
             "uniform in [-1, 1)^3, point weights uniform [0.5, 1.5); big = P * B >= 1e8: 3 calls",
             "# atomic / tiled: raster_smooth_; pullback: raster_pullback_smooth_ (atomic); linear: raster_ (AUTO) of the "
             "same shape; spread: (max - min) / median of the smooth forwards, the larger",
             f"{'grid':<7}{'P':>10}{'B':>4} {'order':<8}{'atomic':>10}{'tiled':>10}{'pullback':>10}{'linear':>10}"
             f"{'spread':>8}  AUTO"]
    for gname, grid in GRIDS:
        if gname not in args.grids.split(","):
            continue
        n_out = len(grid)
        for P in POINTS:
            if P > args.max_points:
                continue
            g = torch.Generator(device=dev).manual_seed(P % 9973)
            pts_r = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
            pw_r = 0.5 + torch.rand((P,), generator=g, device=dev, dtype=dt)
            pts_h, _perm, pw_h = dpr_amd.sort_points(pts_r, pw_r)
            for B in BATCHES:
                d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
                rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
                tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
                bg = torch.as_tensor(d.backgrounds, dtype=dt, device=dev)
                ow = torch.as_tensor(d.weights, dtype=dt, device=dev)
                out = dpr_amd.empty_grid(grid, B, dt, dev)
                ds = dpr_amd.empty_grid(grid, B, dt, dev)
                ds.copy_(torch.randn(ds.shape, generator=g, device=dev, dtype=dt))
                wt = ws(dpr_amd.workspace_bytes_smooth("raster", grid, P, B, n_in, dt, algo="tiled"), dev)
                wl = ws(dpr_amd.workspace_bytes("raster", grid, P, B, n_in, dt), dev)
                reps = 3 if P * B >= 100_000_000 else args.reps
                for order, pts, pw in (("random", pts_r, pw_r), ("hilbert", pts_h, pw_h)):
                    fns = {
                        "atomic": lambda: dpr_amd.raster_smooth_(out, pts, rot, tr, bg, ow, pw, algo="atomic"),
                        "tiled": lambda: dpr_amd.raster_smooth_(out, pts, rot, tr, bg, ow, pw, algo="tiled",
                                                                workspace=wt),
                        "pullback": lambda: dpr_amd.raster_pullback_smooth_(ds, pts, rot, tr, bg, ow, pw),
                        "linear": lambda: dpr_amd.raster_(out, pts, rot, tr, bg, ow, pw, workspace=wl),
                    }
                    ts = timed_in_turn(fns, reps)
                    med = {k: float(np.median(v)) for k, v in ts.items()}
                    spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in ("atomic", "tiled"))
                    auto = dpr_amd.resolve_algo_smooth("raster", grid, P, B, n_in)
                    lines.append(f"{gname:<7}{P:>10}{B:>4} {order:<8}{med['atomic']:10.3f}{med['tiled']:10.3f}"
                                 f"{med['pullback']:10.3f}{med['linear']:10.3f}{spread:8.2f}  {auto}")
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
