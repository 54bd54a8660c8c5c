#!/usr/bin/env python3
"""Smooth sampling (sample_smooth_ / sample_smooth_pullback_) on one MI355X, fp32.

    python tools/sample_smooth_probe.py [--reps 9] [--out profiles/sample_smooth_probe.txt]

For 1e5, 1e6 and 1e7 points -> 256^3, 1e6 points -> 512^2 (one pose each) and 1e5 points x 64 poses -> 128^2, 3-D
points uniform in [-1, 1)^3 as generated: the forward, the pullback (all four gradients) on DPR_ALGO_ATOMIC and on
DPR_ALGO_TILED, and the N-linear `sample_` / `sample_pullback_` (AUTO) of the same shape as a bar.  Inputs and outputs
are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one call (ms)
after a warm-up call of every variant; the variants of a shape are timed in turn within each repetition, so that drift
hits them alike.  The spread column is (max - min) / median over the repetitions, the largest of the three smooth
variants."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402
from tools.smooth_probe import timed_in_turn, ws  # noqa: E402

SHAPES = [("256^3", (256, 256, 256), 100_000, 1), ("256^3", (256, 256, 256), 1_000_000, 1),
          ("256^3", (256, 256, 256), 10_000_000, 1), ("512^2", (512, 512), 1_000_000, 1),
          ("128^2", (128, 128), 100_000, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_smooth_probe.txt"))
    ap.add_argument("--max-points", type=int, default=10_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/sample_smooth_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; "
             "points uniform in [-1, 1)^3 in generation order",
             "# fwd: sample_smooth_; pb_atomic / pb_tiled: sample_smooth_pullback_ (image, points, rotation, "
             "translation); lin_fwd / lin_pb: sample_ / sample_pullback_ (AUTO) of the same shape; spread: "
             "(max - min) / median, the largest of the three smooth variants; AUTO: the smooth pullback's rule",
             f"{'grid':<7}{'P':>10}{'B':>4}{'fwd':>10}{'pb_atomic':>10}{'pb_tiled':>10}{'lin_fwd':>10}{'lin_pb':>10}"
             f"{'spread':>8}  AUTO    lin_pb AUTO"]
    for gname, grid, P, B in SHAPES:
        if P > args.max_points:
            continue
        n_out = len(grid)
        g = torch.Generator(device=dev).manual_seed(P % 9973)
        pts = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
        d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
        rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
        tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
        img = dpr_amd.empty_grid(grid, B, dt, dev)
        img.copy_(torch.randn(img.shape, generator=g, device=dev, dtype=dt))
        dv = torch.randn((B, P), generator=g, device=dev, dtype=dt).t()
        values = torch.empty((B, P), dtype=dt, device=dev).t()
        outs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, dt, dev),
                    ds_dpoints=torch.empty((P, n_in), dtype=dt, device=dev),
                    ds_drotation=torch.empty((B, n_in, n_out), dtype=dt, device=dev).transpose(1, 2),
                    ds_dtranslation=torch.empty((B, n_out), dtype=dt, device=dev))
        wt = ws(dpr_amd.workspace_bytes_sample_smooth("pullback", grid, P, B, n_in, dt, algo="tiled"), dev)
        wl = ws(dpr_amd.workspace_bytes_sample("pullback", grid, P, B, n_in, dt), dev)
        fns = {
            "fwd": lambda: dpr_amd.sample_smooth_(values, img, pts, rot, tr),
            "pb_atomic": lambda: dpr_amd.sample_smooth_pullback_(dv, img, pts, rot, tr, algo="atomic", **outs),
            "pb_tiled": lambda: dpr_amd.sample_smooth_pullback_(dv, img, pts, rot, tr, algo="tiled", workspace=wt,
                                                                **outs),
            "lin_fwd": lambda: dpr_amd.sample_(values, img, pts, rot, tr),
            "lin_pb": lambda: dpr_amd.sample_pullback_(dv, img, pts, rot, tr, workspace=wl, **outs),
        }
        ts = timed_in_turn(fns, args.reps)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in ("fwd", "pb_atomic", "pb_tiled"))
        auto = dpr_amd.resolve_algo_sample_smooth("pullback", grid, P, B, n_in)
        lin_auto = dpr_amd.resolve_algo_sample("pullback", grid, P, B, n_in)
        lines.append(f"{gname:<7}{P:>10}{B:>4}{med['fwd']:10.3f}{med['pb_atomic']:10.3f}{med['pb_tiled']:10.3f}"
                     f"{med['lin_fwd']:10.3f}{med['lin_pb']:10.3f}{spread:8.2f}  {auto:<8}{lin_auto}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
