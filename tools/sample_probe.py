#!/usr/bin/env python3
"""Point sampling forward / pullback beside the existing pullback of the same shape (one MI355X).

    python tools/sample_probe.py [--reps 15] [--out FILE]

Shapes: 10 M Gaussian points -> 256^3 fp32 in generation order and Hilbert-sorted by `sort_points`,
1 M -> 128^3, 10 M -> 512^2 x 8 poses (projections).  For each it times
  * `sample_` (AUTO: the direct gather),
  * `sample_pullback_` (AUTO) with all four gradients,
  * `raster_pullback_` (AUTO) with ds_dout = the image (its ds_dpoint_weight is `sample` for one pose).
Inputs are resident on the device, workspaces allocated once up front.  Times: median over `--reps` of HIP
events around one call (ms).  Prints one table."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("10M -> 256^3 random", 10_000_000, 3, (256, 256, 256), None, False),
          ("10M -> 256^3 sorted", 10_000_000, 3, (256, 256, 256), None, True),
          ("1M -> 128^3", 1_000_000, 3, (128, 128, 128), None, False),
          ("10M -> 512^2 x 8", 10_000_000, 3, (512, 512), 8, False)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/sample_probe.py on {torch.cuda.get_device_name(0)}: median of {a.reps} calls, ms",
             f"{'shape':<22} | {'sample':>8} | {'bwd algo':>8} {'sample pullback':>16} | "
             f"{'raster_pullback algo':>20} {'time':>7}"]
    for name, P, n_in, grid, B, sort in SHAPES:
        rng = np.random.default_rng(0)
        n_out = len(grid)
        pts = torch.as_tensor((0.4 * rng.normal(size=(P, n_in))).astype(np.float32), device=dev)
        if sort:
            pts = dpr_amd.sort_points(pts)[0]
        Bn = B or 1
        R = torch.as_tensor(D.random_rotations(rng, Bn)[:, :n_out].astype(np.float32), device=dev)
        t = torch.as_tensor((0.05 * rng.normal(size=(Bn, n_out))).astype(np.float32), device=dev)
        if B is None:
            R, t = R[0], t[0]
        img = dpr_amd.empty_grid(grid, B, torch.float32, dev)
        img.normal_()
        dv = torch.randn(P, device=dev) if B is None else torch.randn(B, P, device=dev).t()
        values = torch.empty_like(dv)
        algo_b = dpr_amd.resolve_algo_sample("pullback", grid, P, Bn, n_in)
        ws_s = dpr_amd.workspace_bytes_sample("pullback", grid, P, Bn, n_in)
        ws_s = torch.empty(max(ws_s, 1), dtype=torch.uint8, device=dev)
        bufs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, torch.float32, dev),
                    ds_dpoints=torch.empty(P, n_in, device=dev))
        algo_r = dpr_amd.resolve_algo("pullback", grid, P, Bn, n_in, coherent_points=sort)
        ws_r = dpr_amd.workspace_bytes("pullback", grid, P, Bn, n_in, coherent_points=sort)
        ws_r = torch.empty(max(ws_r, 1), dtype=torch.uint8, device=dev)
        t_f = timed(lambda: dpr_amd.sample_(values, img, pts, R, t), a.reps)
        t_b = timed(lambda: dpr_amd.sample_pullback_(dv, img, pts, R, t, workspace=ws_s, **bufs), a.reps)
        t_r = timed(lambda: dpr_amd.raster_pullback_(img, pts, R, t, workspace=ws_r, coherent_points=sort),
                    a.reps)
        lines.append(f"{name:<22} | {t_f:8.3f} | {algo_b:>8} {t_b:16.3f} | {algo_r:>20} {t_r:7.3f}")
        print(lines[-1], flush=True)
        del pts, img, dv, values, bufs, ws_s, ws_r
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
