#!/usr/bin/env python3
"""Per-pose point clouds (raster_clouds_ / raster_pullback_clouds_) on one MI355X, fp32 unless marked.

    python tools/clouds_probe.py [--reps 15] [--out profiles/clouds_probe.txt]

For each shape it times the forward and the pullback of every algorithm of the family, the Python loop of B
single-pose AUTO `raster_` / `raster_pullback_` calls (what a caller does without the family), and the shared-cloud
`raster_` / `raster_pullback_` (AUTO) of the same (grid, P, B) as a bar for the cost per point-pose.  Inputs are
resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one call (ms),
after one warm-up call."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("S1", 3, (128, 128), 256, 20_000, torch.float32),
          ("S2", 3, (256, 256), 64, 100_000, torch.float32),
          ("S3", 3, (64, 64, 64), 32, 100_000, torch.float32),
          ("S4", 3, (256, 256, 256), 4, 2_000_000, torch.float32),
          ("S5", 2, (64, 64), 1024, 4096, torch.float32),
          ("S1-f64", 3, (128, 128), 256, 20_000, torch.float64)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def ws(n, dev):
    return torch.empty(max(n, 256), dtype=torch.uint8, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clouds_probe.txt"))
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    want = args.shapes.split(",")
    lines = [f"# tools/clouds_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X; "
             "clouds 0.3 * randn per pose, point weights uniform [0.5, 1.5)",
             "# loop: B single-pose AUTO raster_ / raster_pullback_ calls; shared: raster_ / raster_pullback_ of one "
             "cloud (AUTO); '-' = the algorithm does not run the shape",
             f"{'shape':<8}{'op':<9}{'atomic':>9}{'tiled':>9}{'chunked':>9}{'loop':>10}{'shared':>9}  AUTO"]
    for name, n_in, grid, B, P, dt in SHAPES:
        if name not in want:
            continue
        n_out = len(grid)
        d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        pts = 0.3 * torch.randn((B, P, n_in), generator=g, device=dev, dtype=dt)
        pw = 0.5 + torch.rand((B, P), generator=g, device=dev, dtype=dt)
        rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
        tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
        bg = torch.as_tensor(d.backgrounds, dtype=dt, device=dev)
        ow = torch.as_tensor(d.weights, dtype=dt, device=dev)
        out = dpr_amd.empty_grid(grid, B, dt, dev)
        ds = dpr_amd.empty_grid(grid, B, dt, dev)
        ds.copy_(torch.randn(ds.shape, generator=g, device=dev, dtype=dt))
        for op in ("raster", "pullback"):
            row = {}
            for algo in ("atomic", "tiled", "chunked"):
                try:
                    w = ws(dpr_amd.workspace_bytes_clouds(op, grid, P, B, n_in, dt, algo=algo), dev)
                except dpr_amd.DprError:
                    row[algo] = None
                    continue
                if op == "raster":
                    f = lambda: dpr_amd.raster_clouds_(out, pts, rot, tr, bg, ow, pw, algo=algo, workspace=w)
                else:
                    f = lambda: dpr_amd.raster_pullback_clouds_(ds, pts, rot, tr, bg, ow, pw, algo=algo, workspace=w)
                row[algo] = timed(f, args.reps)
            w1 = ws(dpr_amd.workspace_bytes(op, grid, P, 1, n_in, dt), dev)
            if op == "raster":
                def loop():
                    for b in range(B):
                        dpr_amd.raster_(out[..., b], pts[b], rot[b], tr[b], bg[b], ow[b], pw[b], workspace=w1)
            else:
                def loop():
                    for b in range(B):
                        dpr_amd.raster_pullback_(ds[..., b], pts[b], rot[b], tr[b], bg[b], ow[b], pw[b], workspace=w1)
            row["loop"] = timed(loop, max(3, args.reps // 3))
            wb = ws(dpr_amd.workspace_bytes(op, grid, P, B, n_in, dt), dev)
            if op == "raster":
                sh = lambda: dpr_amd.raster_(out, pts[0], rot, tr, bg, ow, pw[0], workspace=wb)
            else:
                sh = lambda: dpr_amd.raster_pullback_(ds, pts[0], rot, tr, bg, ow, pw[0], workspace=wb)
            row["shared"] = timed(sh, args.reps)
            auto = dpr_amd.resolve_algo_clouds(op, grid, P, B, n_in, dt)
            fmt = lambda v: f"{'-':>9}" if v is None else f"{v:9.3f}"
            lines.append(f"{name:<8}{op:<9}{fmt(row['atomic'])}{fmt(row['tiled'])}{fmt(row['chunked'])}"
                         f"{row['loop']:10.3f}{row['shared']:9.3f}  {auto}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
