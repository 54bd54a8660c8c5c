#!/usr/bin/env python3
"""DPR_ALGO_ORDERED (bit-reproducible raster and pullback) beside AUTO and DPR_ALGO_ATOMIC (one MI355X, fp32).

    python tools/ordered_probe.py [--reps 15] [--out FILE]

Shapes: 10 M Gaussian points -> 256^3 in generation order and Hilbert-sorted by `sort_points`, 1 M -> 128^3,
1e5 points x 64 poses -> 128^2 (projections), and 10 M points drawn from a Gaussian of sigma = 2 cells on 256^3 --
the heavy-cell cost the contract implies (a cell's sum is serial).  For each it times the forward and the pullback
with algo = "ordered", "auto" and "atomic" and reports the ordered workspaces.  Inputs are resident on the device,
workspaces allocated once up front.  Times: median over `--reps` of HIP events around one call (ms), after a warm-up
call.  Before timing, two ordered forwards are compared bit for bit and the ordered forward with AUTO's norm-wise.
Prints one table."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

# name, P, n_in, grid, B, sigma (in [-1, 1] units), Hilbert-sorted
SHAPES = [("10M -> 256^3 random", 10_000_000, 3, (256, 256, 256), 1, 0.4, False),
          ("10M -> 256^3 sorted", 10_000_000, 3, (256, 256, 256), 1, 0.4, True),
          ("1M -> 128^3", 1_000_000, 3, (128, 128, 128), 1, 0.4, False),
          ("1e5 x 64 -> 128^2", 100_000, 3, (128, 128), 64, 0.4, False),
          ("10M -> 256^3 sigma=2 cells", 10_000_000, 3, (256, 256, 256), 1, 2 * 2.0 / 256, False)]
ALGOS = ("ordered", "auto", "atomic")


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every P (rehearsals)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/ordered_probe.py on {torch.cuda.get_device_name(0)}: fp32, median of {a.reps} calls, ms; "
             f"ws = ordered workspace, MiB",
             f"{'shape':<27} | {'fwd ordered':>11} {'auto':>8} {'(algo)':>9} {'atomic':>8} {'ord/auto':>8} {'ws':>7} | "
             f"{'bwd ordered':>11} {'auto':>8} {'(algo)':>9} {'atomic':>8} {'ord/auto':>8} {'ws':>7}"]
    for name, P, n_in, grid, B, sigma, sort in SHAPES:
        P = max(int(P * a.scale), 1)
        rng = np.random.default_rng(0)
        n_out = len(grid)
        pts = torch.as_tensor((sigma * rng.normal(size=(P, n_in))).astype(np.float32), device=dev)
        if sort:
            pts = dpr_amd.sort_points(pts)[0]
        R = torch.as_tensor(D.random_rotations(rng, B)[:, :n_out].astype(np.float32), device=dev)
        t = torch.as_tensor((0.05 * rng.normal(size=(B, n_out))).astype(np.float32), device=dev)
        pw = torch.as_tensor(rng.uniform(0.5, 1.5, size=P).astype(np.float32), device=dev)
        out = dpr_amd.empty_grid(grid, B, torch.float32, dev)
        g = dpr_amd.empty_grid(grid, B, torch.float32, dev)
        g.normal_()
        bufs = dict(ds_dpoints=torch.empty(P, n_in, device=dev), ds_dpoint_weight=torch.empty(P, device=dev))
        row = {}
        for op in ("raster", "pullback"):
            for algo in ALGOS:
                coh = sort and algo == "auto"
                need = dpr_amd.workspace_bytes(op, grid, P, B, n_in, torch.float32, algo, coherent_points=coh)
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
                if op == "raster":
                    fn = lambda: dpr_amd.raster_(out, pts, R, t, None, None, pw, algo=algo, workspace=ws,  # noqa: E731
                                                 coherent_points=coh)
                else:
                    fn = lambda: dpr_amd.raster_pullback_(g, pts, R, t, None, None, pw, algo=algo,  # noqa: E731
                                                          workspace=ws, coherent_points=coh, **bufs)
                if op == "raster" and algo == "ordered":
                    fn()
                    first = out.clone()
                    fn()
                    torch.cuda.synchronize()
                    assert torch.equal(first, out), f"{name}: two ordered forwards differ"
                if op == "raster" and algo == "auto":
                    fn()
                    torch.cuda.synchronize()
                    err = float((out - first).norm() / first.norm())
                    assert err < 1e-4, f"{name}: ordered and AUTO forwards differ by {err:.2e}"
                row[(op, algo)] = timed(fn, a.reps)
                if algo == "ordered":
                    row[(op, "ws")] = need / 2 ** 20
                del ws
            row[(op, "name")] = dpr_amd.resolve_algo(op, grid, P, B, n_in, coherent_points=sort)
        cells = []
        for op in ("raster", "pullback"):
            cells.append(f"{row[(op, 'ordered')]:11.3f} {row[(op, 'auto')]:8.3f} {'(' + row[(op, 'name')] + ')':>9} "
                         f"{row[(op, 'atomic')]:8.3f} {row[(op, 'ordered')] / row[(op, 'auto')]:8.1f} "
                         f"{row[(op, 'ws')]:7.1f}")
        lines.append(f"{name:<27} | {cells[0]} | {cells[1]}")
        print(lines[-1], flush=True)
        del pts, pw, out, g, bufs, first
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
