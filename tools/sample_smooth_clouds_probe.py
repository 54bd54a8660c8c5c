#!/usr/bin/env python3
"""Smooth sampling at per-pose clouds (sample_smooth_clouds_ / sample_smooth_clouds_pullback_) on one MI355X, fp32.

    python tools/sample_smooth_clouds_probe.py [--reps 9] [--out profiles/sample_smooth_clouds_probe.txt] [--json FILE]

For every (grid, P, B) of tools/smooth_clouds_probe.py's ROWS, B uniform clouds of P points each in generation order:
the forward; the pullback (all four gradients) on DPR_ALGO_ATOMIC, on DPR_ALGO_TILED with the default pose group and
with max_pose_group=1 (pose by pose), and without ds_dimage (the point kernel alone); and the Python loops of B
single-pose `sample_smooth_` and `sample_smooth_pullback_` calls on AUTO that a caller had before this entry point
existed, writing into the same output buffers.  Inputs and outputs are resident on the device, workspaces allocated
once.  Times: median over `--reps` of HIP events around one call (ms) after a warm-up call of every variant; the
variants of a shape are timed in turn within each repetition, so that drift hits them alike.  `spread` is
(max - min) / median over the repetitions, the largest among the five single-call variants.  `--json`: the same rows
as a list of dicts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpr_amd  # noqa: E402
from smooth_clouds_probe import ROWS, timed_in_turn, ws  # noqa: E402
from tests import data as D  # noqa: E402

SINGLE = ("fwd", "pb_atomic", "pb_tiled", "pb_tiled_g1", "pb_noimg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_smooth_clouds_probe.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--grids", default=",".join(sorted({r[0] for r in ROWS})))
    ap.add_argument("--max-points", type=int, default=max(r[2] for r in ROWS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/sample_smooth_clouds_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, "
             "fp32; B clouds of P points uniform in [-1, 1)^3 in generation order, image and ds_dvalues standard normal",
             "# fwd: sample_smooth_clouds_; pb_atomic / pb_tiled / pb_tiled_g1: sample_smooth_clouds_pullback_, all four "
             "gradients (tiled_g1: max_pose_group=1); pb_noimg: the pullback without ds_dimage; loop_fwd / loop_pb: B "
             "calls of sample_smooth_ / sample_smooth_pullback_ (AUTO); group: poses binned together by default; "
             "spread: (max - min) / median of the five single-call variants, the largest; AUTO: the pullback's choice; "
             "loop/fwd = loop_fwd / fwd, loop/AUTO = loop_pb / the pullback AUTO picks",
             f"{'grid':<7}{'P':>9}{'B':>4}{'group':>6}{'fwd':>9}{'pb_atomic':>10}{'pb_tiled':>10}{'pb_tiled_g1':>12}"
             f"{'pb_noimg':>10}{'loop_fwd':>10}{'loop_pb':>10}{'spread':>8}  {'AUTO':<7}{'loop/fwd':>9}{'loop/AUTO':>10}"]
    rows = []
    for gname, grid, P, B in ROWS:
        if gname not in args.grids.split(",") or P > args.max_points:
            continue
        n_out = len(grid)
        g = torch.Generator(device=dev).manual_seed(P % 9973 + B)
        pts = 2 * torch.rand((B, P, n_in), generator=g, device=dev, dtype=dt) - 1
        dv = torch.randn((B, P), generator=g, device=dev, dtype=dt)
        d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
        rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
        tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
        image = dpr_amd.empty_grid(grid, B, dt, dev)
        image.copy_(torch.randn(image.shape, generator=g, device=dev, dtype=dt))
        values = torch.empty((B, P), dtype=dt, device=dev)
        d_img = dpr_amd.empty_grid(grid, B, dt, dev)
        d_pts = torch.empty((B, P, n_in), dtype=dt, device=dev)
        d_rot_cm = torch.empty((B, n_in, n_out), dtype=dt, device=dev)
        d_rot = d_rot_cm.transpose(1, 2)
        d_tr = torch.empty((B, n_out), dtype=dt, device=dev)
        query = dpr_amd._pkg.workspace_bytes_sample_smooth_clouds
        wt = ws(query("pullback", grid, P, B, n_in, dt, "tiled"), dev)
        w1 = ws(query("pullback", grid, P, B, n_in, dt, "tiled", max_pose_group=1), dev)
        wl = ws(dpr_amd.workspace_bytes_sample_smooth("pullback", grid, P, 1, n_in, dt, "tiled"), dev)
        outs = dict(ds_dimage=d_img, ds_dpoints=d_pts, ds_drotation=d_rot, ds_dtranslation=d_tr)
        no_img = dict(ds_dpoints=d_pts, ds_drotation=d_rot, ds_dtranslation=d_tr)
        pull = dpr_amd.sample_smooth_clouds_pullback_

        def loop_fwd():
            for b in range(B):
                dpr_amd.sample_smooth_(values[b], image[..., b], pts[b], rot[b], tr[b])

        def loop_pb():
            for b in range(B):
                dpr_amd.sample_smooth_pullback_(dv[b], image[..., b], pts[b], rot[b], tr[b], ds_dimage=d_img[..., b],
                                                ds_dpoints=d_pts[b], ds_drotation=d_rot[b], ds_dtranslation=d_tr[b],
                                                workspace=wl)

        fns = {
            "fwd": lambda: dpr_amd.sample_smooth_clouds_(values, image, pts, rot, tr),
            "pb_atomic": lambda: pull(dv, image, pts, rot, tr, algo="atomic", **outs),
            "pb_tiled": lambda: pull(dv, image, pts, rot, tr, algo="tiled", workspace=wt, **outs),
            "pb_tiled_g1": lambda: pull(dv, image, pts, rot, tr, algo="tiled", workspace=w1, max_pose_group=1, **outs),
            "pb_noimg": lambda: pull(dv, image, pts, rot, tr, algo="atomic", need=("points", "rotation", "translation"),
                                     **no_img),
            "loop_fwd": loop_fwd,
            "loop_pb": loop_pb,
        }
        ts = timed_in_turn(fns, args.reps)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in SINGLE)
        auto = dpr_amd.resolve_algo_sample_smooth_clouds("pullback", grid, P, B, n_in)
        tiles = int(np.prod([-(-n // e) for n, e in zip(grid, (64, 16) if n_out == 2 else (16, 8, 8))]))
        group = min(B, max(1, (1 << 24) // max(P, tiles)))  # (include/dpr.h, GROUP SIZE)
        lines.append(f"{gname:<7}{P:>9}{B:>4}{group:>6}{med['fwd']:9.3f}{med['pb_atomic']:10.3f}{med['pb_tiled']:10.3f}"
                     f"{med['pb_tiled_g1']:12.3f}{med['pb_noimg']:10.3f}{med['loop_fwd']:10.3f}{med['loop_pb']:10.3f}"
                     f"{spread:8.2f}  {auto:<7}{med['loop_fwd'] / med['fwd']:9.2f}"
                     f"{med['loop_pb'] / med['pb_' + auto]:10.2f}")
        print(lines[-1], flush=True)
        rows.append(dict(grid=list(grid), P=P, B=B, n_in=n_in, group=group, auto=auto, spread=round(spread, 3),
                         ms={k: round(v, 4) for k, v in med.items()}))
        del pts, dv, image, values, d_img, d_pts, d_rot_cm, d_rot, d_tr, wt, w1, wl, outs, no_img
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
