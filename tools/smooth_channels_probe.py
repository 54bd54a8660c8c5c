#!/usr/bin/env python3
"""The smooth splat with C weights per point (raster_smooth_channels_ / raster_pullback_smooth_channels_) on one
MI355X, fp32, against a Python loop of C single-channel smooth calls.

    python tools/smooth_channels_probe.py [--reps 9] [--out profiles/smooth_channels_probe.txt]
                                          [--json tests/golden/smooth_channels_auto.json]
                                          [--variants cb1=PATH,cb4=PATH,b8=PATH]

Shapes: 1e5 x 16 -> 128^2, 1e6 x 1 -> 512^2, 1e5 x 16 -> 128^3, 1e6 x 1 -> 128^3 and 256^3, 1e7 x 1 -> 256^3 (3-D
points, uniform, in generation order, which is random order on the grid); C in {3, 4, 16}.  Columns (ms):

  atomic, tiled   raster_smooth_channels_ on the two algorithms (tiled: the library's channels per workgroup)
  pullback        raster_pullback_smooth_channels_
  loop            C calls of raster_smooth_ on AUTO into the C planes of one pose-major image per channel
  loop_pb         C calls of raster_pullback_smooth_ on AUTO and the sum of their C point, rotation, translation and
                  out_weight gradients (what autograd adds up for the caller of a loop)
  AUTO            the choice of dpr_resolve_algo_smooth_channels for the forward
  loop/AUTO       loop / the fused forward on that choice;  loop_pb/pb: loop_pb / pullback

Inputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one
call after a warm-up call of every variant; the variants of a shape are timed in turn within each repetition, so that
drift hits them alike.  spread: (max - min) / median over the repetitions, the largest of the fused variants.

--variants: other builds of libdpr.so -- ones that differ in the channels a tiled workgroup holds (kSmChTile of
csrc/dpr_smooth_channels.hip), or in how many channels a pullback launch takes -- each measured in a child process of
its own through DPR_LIB_OVERRIDE (same inputs, same protocol; the tiled forward at C = 4 and C = 16 and the pullback at
C = 16, each alone) and reported in further tables next to this build's columns.

--json: the measured rows with the AUTO choices of the library, and the rows of PINS (no times) on both sides of the
AUTO thresholds, as tests/golden/smooth_channels_auto.json holds them."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpr_amd  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("128^2", (128, 128), 100_000, 16), ("512^2", (512, 512), 1_000_000, 1),
          ("128^3", (128, 128, 128), 100_000, 16), ("128^3", (128, 128, 128), 1_000_000, 1),
          ("256^3", (256, 256, 256), 1_000_000, 1), ("256^3", (256, 256, 256), 10_000_000, 1)]
CHANNELS = [3, 4, 16]
# (name, grid, P, B, C): shapes without times on both sides of the AUTO thresholds (P * C = 3e5 on 2-D, 1e5 on 3-D grids)
# and the one-weight shape that bounds the 2-D constant from below
PINS = [("2-D threshold, below", (128, 128), 99_999, 16, 3), ("2-D threshold, at", (128, 128), 75_000, 16, 4),
        ("3-D threshold, below", (128, 128, 128), 24_999, 1, 4), ("3-D threshold, at", (128, 128, 128), 25_000, 1, 4),
        ("one weight, 2-D", (128, 128), 100_000, 16, 1)]
VARIANT_COLUMNS = [("tiled", 4), ("tiled", 16), ("pullback", 16)]


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


def inputs(grid, P, B, C, dev, dt=torch.float32, n_in=3):
    g = torch.Generator(device=dev).manual_seed(P % 9973 + C)
    d = D.make(n_points=4, n_in=n_in, n_out=len(grid), batch=B, grid_n=grid, seed=1)
    a = dict(pts=2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1,
             pw=0.5 + torch.rand((P, C), generator=g, device=dev, dtype=dt),
             rot=torch.as_tensor(d.rotations, dtype=dt, device=dev),
             tr=torch.as_tensor(d.translations, dtype=dt, device=dev),
             ow=torch.as_tensor(d.weights, dtype=dt, device=dev),
             bg=torch.randn((B, C), generator=g, device=dev, dtype=dt))
    a["out"] = dpr_amd.empty_channel_grid(grid, C, B, dt, dev)
    a["wt"] = ws(dpr_amd.workspace_bytes_smooth_channels("raster", grid, P, B, n_in, C, dt, algo="tiled"), dev)
    a["gen"] = g
    return a


def variant_columns(reps):
    """Child mode: VARIANT_COLUMNS on every shape, each alone, as one JSON line of [median ms, spread]."""
    dev = torch.device("cuda:0")
    res = {}
    for gname, grid, P, B in SHAPES:
        for what, C in VARIANT_COLUMNS:
            a = inputs(grid, P, B, C, dev)
            if what == "tiled":
                f = lambda: dpr_amd.raster_smooth_channels_(a["out"], a["pts"], a["rot"], a["tr"], a["pw"], a["bg"],
                                                            a["ow"], algo="tiled", workspace=a["wt"])
            else:
                ds = dpr_amd.empty_channel_grid(grid, C, B, torch.float32, dev)
                ds.copy_(torch.randn(ds.shape, generator=a["gen"], device=dev, dtype=torch.float32))
                f = lambda: dpr_amd.raster_pullback_smooth_channels_(ds, a["pts"], a["rot"], a["tr"], a["pw"], a["bg"],
                                                                     a["ow"])
            ts = timed_in_turn({what: f}, reps)[what]
            res[f"{gname} {P} {B} {what} {C}"] = [float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))]
            del a
            torch.cuda.empty_cache()
    print("VARIANT_COLUMNS " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_channels_probe.txt"))
    ap.add_argument("--json", default="")
    ap.add_argument("--variants", default="")
    ap.add_argument("--variant-columns", action="store_true")
    args = ap.parse_args()
    if args.variant_columns:
        return variant_columns(args.reps)
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/smooth_channels_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; "
             "points uniform in [-1, 1)^3 in generation order, point weights uniform [0.5, 1.5)",
             "# atomic / tiled / pullback: the fused op; loop / loop_pb: C single-channel smooth calls on AUTO (loop_pb "
             "with the sums of the shared gradients); spread: (max - min) / median of the fused variants, the largest",
             f"{'grid':<7}{'P':>10}{'B':>4}{'C':>4}{'atomic':>10}{'tiled':>10}{'pullback':>10}{'loop':>10}"
             f"{'loop_pb':>10}{'spread':>8}  {'AUTO':<7}{'loop/AUTO':>10}{'loop_pb/pb':>11}"]
    rows = []
    for gname, grid, P, B in SHAPES:
        n_out = len(grid)
        for C in CHANNELS:
            a = inputs(grid, P, B, C, dev)
            pts, pw, rot, tr, ow, bg, out, wt = (a[k] for k in ("pts", "pw", "rot", "tr", "ow", "bg", "out", "wt"))
            ds = dpr_amd.empty_channel_grid(grid, C, B, dt, dev)
            ds.copy_(torch.randn(ds.shape, generator=a["gen"], device=dev, dtype=dt))
            # the loop's own buffers: one image per channel, contiguous weights and backgrounds per channel
            outs = [dpr_amd.empty_grid(grid, B, dt, dev) for _ in range(C)]
            dss = [dpr_amd.to_grid_layout(ds[..., c, :]) for c in range(C)]
            pws = [pw[:, c].contiguous() for c in range(C)]
            bgs = [bg[:, c].contiguous() for c in range(C)]
            w1 = ws(dpr_amd.workspace_bytes_smooth("raster", grid, P, B, n_in, dt), dev)

            def loop():
                for c in range(C):
                    dpr_amd.raster_smooth_(outs[c], pts, rot, tr, bgs[c], ow, pws[c], workspace=w1)

            def loop_pb():
                acc = None
                for c in range(C):
                    pb = dpr_amd.raster_pullback_smooth_(dss[c], pts, rot, tr, bgs[c], ow, pws[c])
                    part = (pb.points, pb.rotation, pb.translation, pb.out_weight)
                    acc = part if acc is None else tuple(x + y for x, y in zip(acc, part))
                return acc

            fns = {
                "atomic": lambda: dpr_amd.raster_smooth_channels_(out, pts, rot, tr, pw, bg, ow, algo="atomic"),
                "tiled": lambda: dpr_amd.raster_smooth_channels_(out, pts, rot, tr, pw, bg, ow, algo="tiled",
                                                                 workspace=wt),
                "pullback": lambda: dpr_amd.raster_pullback_smooth_channels_(ds, pts, rot, tr, pw, bg, ow),
                "loop": loop,
                "loop_pb": loop_pb,
            }
            ts = timed_in_turn(fns, args.reps)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in ("atomic", "tiled", "pullback"))
            auto = dpr_amd.resolve_algo_smooth_channels("raster", grid, P, B, n_in, C)
            lines.append(f"{gname:<7}{P:>10}{B:>4}{C:>4}{med['atomic']:10.3f}{med['tiled']:10.3f}"
                         f"{med['pullback']:10.3f}{med['loop']:10.3f}{med['loop_pb']:10.3f}{spread:8.2f}  {auto:<7}"
                         f"{med['loop'] / med[auto]:10.2f}{med['loop_pb'] / med['pullback']:11.2f}")
            print(lines[-1], flush=True)
            rows.append(dict(name=f"{gname} P={P} B={B} C={C}", n_in=n_in, grid=list(grid), P=P, B=B, C=C,
                             auto=dict(raster=auto, pullback=dpr_amd.resolve_algo_smooth_channels(
                                 "pullback", grid, P, B, n_in, C)),
                             ms=dict(raster=dict(atomic=round(med["atomic"], 4), tiled=round(med["tiled"], 4)))))
            del a, out, ds, outs, dss, wt, w1
            torch.cuda.empty_cache()
    if args.variants:
        col = {"tiled": 5, "pullback": 6}
        this = {}
        for line in lines[3:]:
            f = line.split()
            for what, C in VARIANT_COLUMNS:
                if int(f[3]) == C:
                    this[f"{f[0]} {f[1]} {f[2]} {what} {C}"] = float(f[col[what]])
        cols = {}
        for item in args.variants.split(","):
            name, path = item.split("=", 1)
            env = dict(os.environ, DPR_LIB_OVERRIDE=os.path.abspath(path))
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant-columns", "--reps",
                                  str(args.reps)], env=env, capture_output=True, text=True, check=True)
            got = [ln for ln in run.stdout.splitlines() if ln.startswith("VARIANT_COLUMNS ")]
            cols[name] = json.loads(got[-1][len("VARIANT_COLUMNS "):])
        for what, C in VARIANT_COLUMNS:
            lines += ["", f"# {what} at C = {C}: `this` is the column of the first table; the others are the builds of "
                      "--variants, each timed alone in a process of its own (ms, spread)",
                      f"{'grid':<7}{'P':>10}{'B':>4}{'this':>10}" + "".join(f"{n:>16}" for n in cols)]
            for gname, grid, P, B in SHAPES:
                key = f"{gname} {P} {B} {what} {C}"
                lines.append(f"{gname:<7}{P:>10}{B:>4}{this[key]:10.3f}"
                             + "".join(f"{cols[n][key][0]:10.3f} {cols[n][key][1]:5.2f}" for n in cols))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        for name, grid, P, B, C in PINS:
            rows.append(dict(name=name, n_in=n_in, grid=list(grid), P=P, B=B, C=C,
                             auto={op: dpr_amd.resolve_algo_smooth_channels(op, grid, P, B, n_in, C)
                                   for op in ("raster", "pullback")}))
        table = dict(source="profiles/smooth_channels_probe.txt (tools/smooth_channels_probe.py, fp32, one MI355X; ms, "
                            "median); rows without ms pin the thresholds of dpr_resolve_algo_smooth_channels",
                     shapes=rows)
        with open(args.json, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
