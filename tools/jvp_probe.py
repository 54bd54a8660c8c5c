#!/usr/bin/env python3
"""Forward-mode derivative of raster (raster_jvp_) beside the forward of the same shape (one MI355X).

    python tools/jvp_probe.py [--reps 15] [--out profiles/jvp_probe.txt]

Shapes: 10 M Gaussian points -> 256^3 fp32 in generation order and Hilbert-sorted by `sort_points`, 1 M -> 128^3,
10 M -> 512^2 x 8 poses (projections).  Tangents: points, rotation, translation and point weights, K = 1, 4, 12.
For each (shape, K) it times `raster_jvp_` on DPR_ALGO_TILED and DPR_ALGO_ATOMIC, `raster_` (AUTO) of the same
shape, and K single-tangent calls on AUTO's algorithm against the one K-tangent call.  Inputs are resident on
the device, workspaces allocated once up front.  Times: median over `--reps` of HIP events around one call (ms),
after one warm-up call; a variant slower than 200 ms per call is timed over 3 calls instead (marked *)."""
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
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
        if i == 0 and ts[0] > 200.0 and reps > 3:
            return float(np.median(ts + [timed_once(fn) for _ in range(2)])), True
    return float(np.median(ts)), False


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jvp_probe.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/jvp_probe.py: fp32, median of {args.reps} calls after a warm-up (ms); "
             "one MI355X",
             "# K-call vs K x 1: one K-tangent call on AUTO's algorithm against K single-tangent calls on it; "
             "* = timed over 3 calls (> 200 ms each)",
             f"{'shape':<22}{'K':>3}  {'AUTO':<7}{'tiled':>9}{'atomic':>11}{'raster_':>9}{'K-call':>9}"
             f"{'K x 1':>9}  AUTO faster?"]
    for name, P, n_in, grid, B, sort in SHAPES:
        d = D.make(n_points=16, n_in=n_in, n_out=len(grid), batch=B or 1, grid_n=grid, seed=1)
        rng = np.random.default_rng(2)
        pts = torch.as_tensor(0.4 * rng.normal(size=(P, n_in)), dtype=torch.float32, device=dev)
        if sort:
            pts = dpr_amd.sort_points(pts)[0]
        rot = torch.as_tensor(d.rotations[0] if B is None else d.rotations, dtype=torch.float32, device=dev)
        trans = torch.as_tensor(d.translations[0] if B is None else d.translations, dtype=torch.float32, device=dev)
        pw = torch.rand(P, device=dev)
        Bn = B or 1
        out = dpr_amd.raster(grid, pts, rot, trans, None, None, pw)
        ws_r = torch.empty(max(dpr_amd.workspace_bytes("raster", grid, P, Bn, n_in), 16), dtype=torch.uint8,
                           device=dev)
        t_raster, _ = timed(lambda: dpr_amd.raster_(out, pts, rot, trans, None, None, pw, workspace=ws_r),
                            args.reps)
        ws = torch.empty(max(dpr_amd.workspace_bytes_jvp(grid, P, Bn, n_in, 1, algo="tiled"), 16), dtype=torch.uint8,
                         device=dev)
        for K in (1, 4, 12):
            pose = () if B is None else (B,)
            tk = dict(points_dot=torch.randn(K, P, n_in, device=dev),
                      rotation_dot=torch.randn((K,) + pose + tuple(rot.shape[-2:]), device=dev),
                      translation_dot=torch.randn((K,) + pose + (len(grid),), device=dev),
                      point_weight_dot=torch.randn(K, P, device=dev))
            out_dot = dpr_amd.empty_channel_grid(grid, K, B, torch.float32, dev)
            auto = dpr_amd.resolve_algo_jvp(grid, P, Bn, n_in, K)
            t = {}
            for algo in ("tiled", "atomic"):
                t[algo] = timed(lambda: dpr_amd.raster_jvp_(out_dot, pts, rot, trans, None, None, pw, **tk,
                                                            tangents=K, algo=algo, workspace=ws), args.reps)
            one = {n: v[0] for n, v in tk.items()}
            out1 = dpr_amd.empty_grid(grid, B, torch.float32, dev)

            def singles():
                for _ in range(K):
                    dpr_amd.raster_jvp_(out1, pts, rot, trans, None, None, pw, **one, algo=auto, workspace=ws)

            t_single, _ = timed(singles, args.reps)
            other = "atomic" if auto == "tiled" else "tiled"
            faster = "yes" if t[auto][0] <= t[other][0] else "no"
            star = lambda x: f"{x[0]:.3f}" + ("*" if x[1] else "")
            lines.append(f"{name:<22}{K:>3}  {auto:<7}{star(t['tiled']):>9}{star(t['atomic']):>11}"
                         f"{t_raster:>9.3f}{t[auto][0]:>9.3f}{t_single:>9.3f}  {faster}")
            print(lines[-1], flush=True)
            del tk, out_dot
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
