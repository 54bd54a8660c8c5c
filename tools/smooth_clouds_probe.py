#!/usr/bin/env python3
"""The smooth splat of per-pose clouds (raster_smooth_clouds_ / raster_pullback_smooth_clouds_) on one MI355X, fp32.

    python tools/smooth_clouds_probe.py [--reps 9] [--out profiles/smooth_clouds_probe.txt] [--json FILE]

For every (grid, P, B) of ROWS, B uniform clouds of P points each in generation order: the forward on DPR_ALGO_ATOMIC,
on DPR_ALGO_TILED with the default pose group and with max_pose_group=1 (pose by pose), and as the Python loop of B
single-pose `raster_smooth_` calls on AUTO that a caller had before this entry point existed; the atomic pullback and
the same loop of `raster_pullback_smooth_`.  Inputs are resident on the device, workspaces allocated once.  Times:
median over `--reps` of HIP events around one call (ms) after a warm-up call of every variant; the variants of a shape
are timed in turn within each repetition, so that drift hits them alike.  `spread` is (max - min) / median over the
repetitions, the largest among the three single-call forwards.  `--json`: the same rows as a list of dicts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

ROWS = ([("128^2", (128, 128), P, B) for P in (10_000, 100_000, 1_000_000) for B in (16, 64)]
        + [("512^2", (512, 512), P, 16) for P in (100_000, 1_000_000)]
        + [(name, (n, n, n), P, B) for name, n in (("128^3", 128), ("256^3", 256))
           for P in (100_000, 1_000_000) for B in (4, 16)]
        # around the AUTO thresholds (group * P of 5e5 for 2-D grids, 1e5 for 3-D grids)
        + [("128^2", (128, 128), 10_000, 32), ("128^2", (128, 128), 30_000, 16), ("512^2", (512, 512), 30_000, 16),
           ("128^3", (128,) * 3, 10_000, 4), ("128^3", (128,) * 3, 10_000, 16), ("128^3", (128,) * 3, 30_000, 4),
           ("256^3", (256,) * 3, 10_000, 4), ("256^3", (256,) * 3, 10_000, 16), ("256^3", (256,) * 3, 30_000, 4)])
FORWARDS = ("atomic", "tiled", "tiled_g1")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_clouds_probe.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--grids", default=",".join(sorted({r[0] for r in ROWS})))
    ap.add_argument("--max-points", type=int, default=max(r[2] for r in ROWS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/smooth_clouds_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; B "
             "clouds of P points uniform in [-1, 1)^3 in generation order, point weights uniform [0.5, 1.5)",
             "# atomic / tiled / tiled_g1: raster_smooth_clouds_ (tiled_g1: max_pose_group=1); loop: B calls of "
             "raster_smooth_ (AUTO); pullback: raster_pullback_smooth_clouds_; loop_pb: B calls of "
             "raster_pullback_smooth_; group: poses binned together by default; spread: (max - min) / median of the "
             "three single-call forwards, the largest",
             f"{'grid':<7}{'P':>9}{'B':>4}{'group':>6}{'atomic':>10}{'tiled':>10}{'tiled_g1':>10}{'loop':>10}"
             f"{'pullback':>10}{'loop_pb':>10}{'spread':>8}  {'AUTO':<7}{'loop/tiled':>11}{'loop/AUTO':>10}"]
    rows = []
    for gname, grid, P, B in ROWS:
        if gname not in args.grids.split(",") or P > args.max_points:
            continue
        n_out = len(grid)
        g = torch.Generator(device=dev).manual_seed(P % 9973 + B)
        pts = 2 * torch.rand((B, P, n_in), generator=g, device=dev, dtype=dt) - 1
        pw = 0.5 + torch.rand((B, P), generator=g, device=dev, dtype=dt)
        d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
        rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
        tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
        bg = torch.as_tensor(d.backgrounds, dtype=dt, device=dev)
        ow = torch.as_tensor(d.weights, dtype=dt, device=dev)
        bg_l, ow_l = [float(x) for x in d.backgrounds], [float(x) for x in d.weights]
        out = dpr_amd.empty_grid(grid, B, dt, dev)
        ds = dpr_amd.empty_grid(grid, B, dt, dev)
        ds.copy_(torch.randn(ds.shape, generator=g, device=dev, dtype=dt))
        wt = ws(dpr_amd.workspace_bytes_smooth_clouds("raster", grid, P, B, n_in, dt, "tiled"), dev)
        w1 = ws(dpr_amd.workspace_bytes_smooth_clouds("raster", grid, P, B, n_in, dt, "tiled", max_pose_group=1), dev)
        wl = ws(dpr_amd.workspace_bytes_smooth("raster", grid, P, 1, n_in, dt, "tiled"), dev)

        def loop():
            for b in range(B):
                dpr_amd.raster_smooth_(out[..., b], pts[b], rot[b], tr[b], bg_l[b], ow_l[b], pw[b], workspace=wl)

        def loop_pb():
            for b in range(B):
                dpr_amd.raster_pullback_smooth_(ds[..., b], pts[b], rot[b], tr[b], bg_l[b], ow_l[b], pw[b])

        fns = {
            "atomic": lambda: dpr_amd.raster_smooth_clouds_(out, pts, rot, tr, bg, ow, pw, algo="atomic"),
            "tiled": lambda: dpr_amd.raster_smooth_clouds_(out, pts, rot, tr, bg, ow, pw, algo="tiled", workspace=wt),
            "tiled_g1": lambda: dpr_amd.raster_smooth_clouds_(out, pts, rot, tr, bg, ow, pw, algo="tiled",
                                                              workspace=w1, max_pose_group=1),
            "loop": loop,
            "pullback": lambda: dpr_amd.raster_pullback_smooth_clouds_(ds, pts, rot, tr, bg, ow, pw),
            "loop_pb": loop_pb,
        }
        ts = timed_in_turn(fns, args.reps)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in FORWARDS)
        auto = dpr_amd.resolve_algo_smooth_clouds("raster", grid, P, B, n_in)
        tiles = int(np.prod([-(-n // e) for n, e in zip(grid, (64, 16) if n_out == 2 else (16, 8, 8))]))
        group = min(B, max(1, (1 << 24) // max(P, tiles)))  # (include/dpr.h, GROUP SIZE)
        lines.append(f"{gname:<7}{P:>9}{B:>4}{group:>6}{med['atomic']:10.3f}{med['tiled']:10.3f}"
                     f"{med['tiled_g1']:10.3f}{med['loop']:10.3f}{med['pullback']:10.3f}{med['loop_pb']:10.3f}"
                     f"{spread:8.2f}  {auto:<7}{med['loop'] / med['tiled']:11.2f}{med['loop'] / med[auto]:10.2f}")
        print(lines[-1], flush=True)
        rows.append(dict(grid=list(grid), P=P, B=B, n_in=n_in, group=group, auto=auto, spread=round(spread, 3),
                         ms={k: round(v, 4) for k, v in med.items()}))
        del pts, pw, out, ds, wt, w1, wl
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
