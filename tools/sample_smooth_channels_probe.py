#!/usr/bin/env python3
"""Smooth sampling of C-channel images (sample_smooth_channels_ / sample_smooth_channels_pullback_) on one MI355X,
fp32.

    python tools/sample_smooth_channels_probe.py [--reps 9] [--out profiles/sample_smooth_channels_probe.txt]
                                                 [--grids 128^2,512^2,128^3,256^3] [--channels 3,4,16] [--append]
                                                 [--note TEXT]

One run under `timeout`.  The shapes are those of profiles/smooth_channels_probe.txt (tools/smooth_channels_probe.py:
SHAPES, CHANNELS), uniform clouds in generation order ("random"), and the 1e6 -> 256^3 rows once more on the cloud
sorted along the Hilbert curve (dpr_amd.sort_points, "hilbert").  Per row:

  fwd                     sample_smooth_channels_ (DPR_ALGO_ATOMIC, the only forward)
  pb_atomic / pb_tiled    sample_smooth_channels_pullback_ with all four gradients on either algorithm
  pb_geom                 the same without "image" (need = points, rotation, translation): the point kernel alone
  loop / loop_pb          the composite the op replaces, in the same process on the same build: C calls of
                          sample_smooth_ / sample_smooth_pullback_ on AUTO on the planes (copied out beforehand, outside
                          the timing; ds_dvalues likewise); the pullback writes per-plane buffers and the 3 (C - 1)
                          additions of the geometric gradients are timed with it

Inputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one
call (ms) after a warm-up call of every variant; the variants of a row are timed in turn within each repetition
(timed_in_turn of tools/smooth_channels_probe.py), so that drift hits them alike.  `spread` is (max - min) / median
over the repetitions, the largest among the four fused calls."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dpr_amd  # noqa: E402
from dpr_amd import _lib  # noqa: E402
from smooth_channels_probe import CHANNELS, SHAPES, timed_in_turn, ws  # noqa: E402
from tests import data as D  # noqa: E402

FUSED = ("fwd", "pb_atomic", "pb_tiled", "pb_geom")
GEOM = ("points", "rotation", "translation")
HILBERT = ("256^3", 1_000_000)  # the rows that run on the sorted cloud as well


def query(grid, P, B, C, n_in):
    """dpr_workspace_bytes_sample_smooth_channels_ex_f32 for the tiled pullback (the family has no public query)."""
    a = np.asarray(grid, dtype=np.int64)
    return int(dpr_amd.lib().dpr_workspace_bytes_sample_smooth_channels_ex_f32(
        _lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, len(grid), a.ctypes.data_as(ctypes.c_void_p), P, B, C))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_smooth_channels_probe.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--grids", default="128^2,512^2,128^3,256^3")
    ap.add_argument("--channels", default=",".join(str(c) for c in CHANNELS))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = []
    if not args.append:
        lines += [f"# tools/sample_smooth_channels_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, "
                  "fp32; P points uniform in [-1, 1)^3 in generation order (random) or sorted along the Hilbert curve "
                  "(hilbert), image and ds_dvalues standard normal",
                  "# fwd: sample_smooth_channels_; pb_atomic / pb_tiled: sample_smooth_channels_pullback_, four "
                  "gradients; pb_geom: without ds_dimage; loop / loop_pb: C calls of sample_smooth_ / "
                  "sample_smooth_pullback_ (AUTO) on the planes, loop_pb with the sums of the geometric gradients; "
                  "spread: (max - min) / median of the four fused calls, the largest; AUTO: the pullback's algorithm"]
    if args.note:
        lines.append(f"# {args.note}")
    lines.append(f"{'grid':<7}{'P':>9}{'B':>4}{'C':>4} {'order':<8}{'fwd':>8}{'pb_atomic':>10}{'pb_tiled':>9}{'pb_geom':>9}"
                 f"{'loop':>9}{'loop_pb':>9}{'spread':>8}  {'AUTO':<7}{'loop/fwd':>9}{'loop_pb/AUTO':>13}{'other/AUTO':>11}")
    print("\n".join(lines), flush=True)
    for gname, grid, P, B in SHAPES:
        if gname not in args.grids.split(","):
            continue
        n_out = len(grid)
        for C in (int(c) for c in args.channels.split(",")):
            g = torch.Generator(device=dev).manual_seed(P % 9973 + B + C)
            pts0 = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
            d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
            rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
            tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
            image = dpr_amd.empty_channel_grid(grid, C, B, dt, dev)
            image.copy_(torch.randn(image.shape, generator=g, device=dev, dtype=dt))
            dv = torch.randn((B, P, C), generator=g, device=dev, dtype=dt).permute(1, 2, 0)
            values = torch.empty((B, P, C), device=dev, dtype=dt).permute(1, 2, 0)
            e = lambda *s: torch.empty(s, device=dev, dtype=dt)
            outs = dict(ds_dimage=dpr_amd.empty_channel_grid(grid, C, B, dt, dev), ds_dpoints=e(P, n_in),
                        ds_drotation=e(B, n_in, n_out).transpose(1, 2), ds_dtranslation=e(B, n_out))
            geom = {k: v for k, v in outs.items() if k != "ds_dimage"}
            wt = ws(query(grid, P, B, C, n_in), dev)
            # the loop's planes, value gradients and per-plane outputs
            planes = [dpr_amd.to_grid_layout(image[..., c, :]) for c in range(C)]
            dvs = [dv[:, c, :].t().contiguous().t() for c in range(C)]
            vals = [torch.empty((B, P), device=dev, dtype=dt).t() for _ in range(C)]
            per = [dict(ds_dimage=dpr_amd.empty_grid(grid, B, dt, dev), ds_dpoints=e(P, n_in),
                        ds_drotation=e(B, n_in, n_out).transpose(1, 2), ds_dtranslation=e(B, n_out)) for _ in range(C)]
            wl = ws(dpr_amd.workspace_bytes_sample_smooth("pullback", grid, P, B, n_in, dt), dev)
            orders = ("random", "hilbert") if (gname, P) == HILBERT else ("random",)
            for order in orders:
                pts = dpr_amd.sort_points(pts0)[0] if order == "hilbert" else pts0

                def loop_fwd():
                    for c in range(C):
                        dpr_amd.sample_smooth_(vals[c], planes[c], pts, rot, tr)

                def loop_pb():
                    for c in range(C):
                        dpr_amd.sample_smooth_pullback_(dvs[c], planes[c], pts, rot, tr, workspace=wl, **per[c])
                    for c in range(1, C):
                        for k in ("ds_dpoints", "ds_drotation", "ds_dtranslation"):
                            per[0][k].add_(per[c][k])

                pull = lambda **kw: dpr_amd.sample_smooth_channels_pullback_(dv, image, pts, rot, tr, **kw)
                fns = {
                    "fwd": lambda: dpr_amd.sample_smooth_channels_(values, image, pts, rot, tr),
                    "pb_atomic": lambda: pull(algo="atomic", **outs),
                    "pb_tiled": lambda: pull(algo="tiled", workspace=wt, **outs),
                    "pb_geom": lambda: pull(algo="atomic", need=GEOM, **geom),
                    "loop": loop_fwd, "loop_pb": loop_pb,
                }
                ts = timed_in_turn(fns, args.reps)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in FUSED)
                auto = dpr_amd.resolve_algo_sample_smooth_channels("pullback", grid, P, B, n_in, C)
                other = "pb_atomic" if auto == "tiled" else "pb_tiled"
                lines.append(f"{gname:<7}{P:>9}{B:>4}{C:>4} {order:<8}{med['fwd']:8.3f}{med['pb_atomic']:10.3f}"
                             f"{med['pb_tiled']:9.3f}{med['pb_geom']:9.3f}{med['loop']:9.3f}{med['loop_pb']:9.3f}"
                             f"{spread:8.2f}  {auto:<7}{med['loop'] / med['fwd']:9.2f}"
                             f"{med['loop_pb'] / med['pb_' + auto]:13.2f}{med[other] / med['pb_' + auto]:11.2f}")
                print(lines[-1], flush=True)
            del pts0, image, dv, values, outs, geom, wt, planes, dvs, vals, per, wl
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
