#!/usr/bin/env python3
"""Multi-channel forward / pullback against C single-channel calls (one MI355X).

    python tools/channels_probe.py [--reps 20] [--out FILE]

For C in {1, 3, 4} and three shapes -- 10 M random (Gaussian) points -> 256^3 fp32, 1 M -> 128^3, 10 M ->
512^2 x 8 poses (projections) -- times
  * `raster_channels` (AUTO) against C single-channel `raster_` calls (AUTO) that write the same planes
    (a batched call writes into C separate (grid, B) buffers: the single-channel API has no plane stride);
  * `raster_pullback_channels_` (AUTO = the direct kernel) against C single-channel `raster_pullback_`
    calls (AUTO) plus the C - 1 additions of their ds_dpoints / per-pose sums.
Inputs are resident on the device, the workspaces preallocated by torch's caching allocator (one warm-up
call each).  Times: median over `--reps` of HIP events around one call (ms).  Prints one table."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("10M -> 256^3", 10_000_000, 3, (256, 256, 256), None),
          ("1M -> 128^3", 1_000_000, 3, (128, 128, 128), None),
          ("10M -> 512^2 x 8", 10_000_000, 3, (512, 512), 8)]


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, P, n_in, grid, B in SHAPES:
        rng = np.random.default_rng(0)
        n_out = len(grid)
        pts = torch.as_tensor((0.4 * rng.normal(size=(P, n_in))).astype(np.float32), device=dev)
        if B is None:
            R = torch.as_tensor(D.random_rotations(rng, 1)[0][:n_out].astype(np.float32), device=dev)
            t = torch.as_tensor((0.05 * rng.normal(size=n_out)).astype(np.float32), device=dev)
            ow = 1.0
        else:
            R = torch.as_tensor(D.random_rotations(rng, B)[:, :n_out].astype(np.float32), device=dev)
            t = torch.as_tensor((0.05 * rng.normal(size=(B, n_out))).astype(np.float32), device=dev)
            ow = torch.ones(B, device=dev)
        for C in (1, 3, 4):
            pw = torch.rand(P, C, device=dev) + 0.5
            cols = [pw[:, c].contiguous() for c in range(C)]
            bg = torch.zeros((C,) if B is None else (B, C), device=dev)
            out = dpr_amd.empty_channel_grid(grid, C, B, torch.float32, dev)
            singles = [dpr_amd.empty_grid(grid, B, torch.float32, dev) for _ in range(C)]
            g = dpr_amd.empty_channel_grid(grid, C, B, torch.float32, dev)
            g.normal_()
            g_single = [dpr_amd.to_grid_layout(g.select(n_out, c)) for c in range(C)]
            algo_f = dpr_amd.resolve_algo_channels("raster", grid, P, B or 1, n_in, C)
            algo_b = dpr_amd.resolve_algo_channels("pullback", grid, P, B or 1, n_in, C)
            auto_f = dpr_amd.resolve_algo("raster", grid, P, B or 1, n_in)
            auto_b = dpr_amd.resolve_algo("pullback", grid, P, B or 1, n_in)
            bgc = lambda c: 0.0 if B is None else bg[:, c].contiguous()

            def fwd_ch():
                dpr_amd.raster_channels_(out, pts, R, t, pw, bg, ow)

            def fwd_single():
                for c in range(C):
                    dpr_amd.raster_(singles[c], pts, R, t, bgc(c), ow, cols[c])

            def bwd_ch():
                dpr_amd.raster_pullback_channels_(g, pts, R, t, pw, bg, ow)

            def bwd_single():
                acc = None
                for c in range(C):
                    r = dpr_amd.raster_pullback_(g_single[c], pts, R, t, bgc(c), ow, cols[c])
                    parts = (r.points, r.rotation, r.translation, r.out_weight)
                    acc = list(parts) if acc is None else [x + y for x, y in zip(acc, parts)]

            tf, tfs = timed(fwd_ch, a.reps), timed(fwd_single, a.reps)
            tb, tbs = timed(bwd_ch, a.reps), timed(bwd_single, a.reps)
            rows.append((name, C, algo_f, auto_f, tf, tfs, algo_b, auto_b, tb, tbs))
            del out, singles, g, g_single, pw, cols
            torch.cuda.empty_cache()
    lines = [f"# tools/channels_probe.py on {torch.cuda.get_device_name(0)}: median of {a.reps} calls, ms",
             f"{'shape':18s} {'C':>2s} | {'fwd algo':>8s} {'channels':>9s} {'C x single':>10s} {'ratio':>6s}"
             f" | {'bwd algo':>8s} {'channels':>9s} {'C x single':>10s} {'ratio':>6s}"]
    for name, C, af, sf, tf, tfs, ab, sb, tb, tbs in rows:
        lines.append(f"{name:18s} {C:2d} | {af:>8s} {tf:9.3f} {tfs:10.3f} {tfs / tf:6.2f}"
                     f" | {ab:>8s} {tb:9.3f} {tbs:10.3f} {tbs / tb:6.2f}")
    lines.append("(ratio = C single-channel calls / one channel call: > 1 means the channel path is faster; the "
                 "single calls run AUTO: " + ", ".join(sorted({f"{r[0]}: fwd {r[3]} / bwd {r[7]}" for r in rows})) + ")")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
