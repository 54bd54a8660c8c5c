#!/usr/bin/env python3
"""The forward-mode derivative of the smooth splat (raster_smooth_jvp_) on one MI355X, fp32.

    python tools/smooth_jvp_probe.py [--reps 9] [--out profiles/smooth_jvp_probe.txt]
                                     [--json tests/golden/smooth_jvp_auto.json]

For 1e5, 1e6 and 1e7 points -> 256^3, 1e6 -> 512^2, 1e7 -> 128^3 (one pose each) and 1e5 points x 16 poses -> 128^2,
3-D points uniform in [-1, 1)^3 as generated, and K = 1, 4, 12 tangents (all five point / pose tangents and the
background tangent given): the JVP on DPR_ALGO_ATOMIC and on DPR_ALGO_TILED, and next to them two bars of code this
op does not touch -- `raster_smooth_` on the same algorithm (one plane) and the N-linear `raster_jvp_` (AUTO) with the
same K.  Inputs and outputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP
events around one call (ms) after a warm-up call of every variant; the variants of a shape are timed in turn within
each repetition, so that drift hits them alike.  /plane: the JVP's time divided by K; x fwd: that over the smooth
forward on the same algorithm; x lin: the JVP's time over the linear JVP's.  spread: (max - min) / median over the
repetitions, the larger of the two smooth JVPs.  The rows also go to a JSON table (shape, K, atomic ms, tiled ms,
AUTO's choice) that tests/test_smooth_jvp_abi.py holds dpr_resolve_algo_smooth_jvp to."""
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
from tools.smooth_probe import timed_in_turn, ws  # noqa: E402

SHAPES = [("256^3", (256, 256, 256), 100_000, 1), ("256^3", (256, 256, 256), 1_000_000, 1),
          ("256^3", (256, 256, 256), 10_000_000, 1), ("512^2", (512, 512), 1_000_000, 1),
          ("128^3", (128, 128, 128), 10_000_000, 1), ("128^2", (128, 128), 100_000, 16)]
TANGENTS = [1, 4, 12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_jvp_probe.txt"))
    ap.add_argument("--json", default=os.path.join(ROOT, "tests", "golden", "smooth_jvp_auto.json"))
    ap.add_argument("--max-points", type=int, default=10_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = [f"# tools/smooth_jvp_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; points "
             "uniform in [-1, 1)^3 in generation order, point weights uniform [0.5, 1.5), tangents N(0, 1)",
             "# atomic / tiled: raster_smooth_jvp_ with K tangents; fwd_a / fwd_t: raster_smooth_ (one plane) on the "
             "same algorithm; lin: raster_jvp_ (AUTO) with K tangents; /plane: JVP ms / K; x fwd: /plane over the "
             "smooth forward; x lin: JVP over the linear JVP; spread: (max - min) / median, the larger of the two JVPs",
             f"{'grid':<7}{'P':>10}{'B':>4}{'K':>4}{'atomic':>10}{'tiled':>10}{'fwd_a':>9}{'fwd_t':>9}{'lin':>10}"
             f"{'a/plane':>9}{'t/plane':>9}{'a x fwd':>9}{'t x fwd':>9}{'a x lin':>9}{'t x lin':>9}{'spread':>8}  AUTO"]
    rows = []
    for gname, grid, P, B in SHAPES:
        if P > args.max_points:
            continue
        n_out = len(grid)
        g = torch.Generator(device=dev).manual_seed(P % 9973)
        pts = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
        pw = 0.5 + torch.rand((P,), generator=g, device=dev, dtype=dt)
        d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=1)
        rot = torch.as_tensor(d.rotations, dtype=dt, device=dev)
        tr = torch.as_tensor(d.translations, dtype=dt, device=dev)
        bg = torch.as_tensor(d.backgrounds, dtype=dt, device=dev)
        ow = torch.as_tensor(d.weights, dtype=dt, device=dev)
        out = dpr_amd.empty_grid(grid, B, dt, dev)
        wf = ws(dpr_amd.workspace_bytes_smooth("raster", grid, P, B, n_in, dt, algo="tiled"), dev)
        for K in TANGENTS:
            rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=dt)
            tan = dict(points_dot=rnd(K, P, n_in), rotation_dot=rnd(K, B, n_out, n_in), translation_dot=rnd(K, B, n_out),
                       background_dot=rnd(K, B), out_weight_dot=rnd(K, B), point_weight_dot=rnd(K, P))
            out_dot = dpr_amd.empty_channel_grid(grid, K, B, dt, dev)
            wt = ws(dpr_amd.workspace_bytes_smooth_jvp(grid, P, B, n_in, K, dt, algo="tiled"), dev)
            wl = ws(dpr_amd.workspace_bytes_jvp(grid, P, B, n_in, K, dt), dev)
            fns = {
                "atomic": lambda: dpr_amd.raster_smooth_jvp_(out_dot, pts, rot, tr, bg, ow, pw, tangents=K,
                                                             algo="atomic", **tan),
                "tiled": lambda: dpr_amd.raster_smooth_jvp_(out_dot, pts, rot, tr, bg, ow, pw, tangents=K,
                                                            algo="tiled", workspace=wt, **tan),
                "fwd_a": lambda: dpr_amd.raster_smooth_(out, pts, rot, tr, bg, ow, pw, algo="atomic"),
                "fwd_t": lambda: dpr_amd.raster_smooth_(out, pts, rot, tr, bg, ow, pw, algo="tiled", workspace=wf),
                "lin": lambda: dpr_amd.raster_jvp_(out_dot, pts, rot, tr, bg, ow, pw, tangents=K, workspace=wl, **tan),
            }
            ts = timed_in_turn(fns, args.reps)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in ("atomic", "tiled"))
            auto = dpr_amd.resolve_algo_smooth_jvp(grid, P, B, n_in, K)
            a, t = med["atomic"], med["tiled"]
            lines.append(f"{gname:<7}{P:>10}{B:>4}{K:>4}{a:10.3f}{t:10.3f}{med['fwd_a']:9.3f}{med['fwd_t']:9.3f}"
                         f"{med['lin']:10.3f}{a / K:9.3f}{t / K:9.3f}{a / K / med['fwd_a']:9.2f}"
                         f"{t / K / med['fwd_t']:9.2f}{a / med['lin']:9.2f}{t / med['lin']:9.2f}{spread:8.2f}  {auto}")
            print(lines[-1], flush=True)
            rows.append(dict(name=f"{P} -> {gname} x {B}", grid=list(grid), n_in=n_in, P=P, B=B, K=K,
                             ms=dict(atomic=round(a, 4), tiled=round(t, 4)), auto=auto))
            del tan, out_dot
    for path, text in ((args.out, "\n".join(lines) + "\n"),
                       (args.json, json.dumps(dict(source="tools/smooth_jvp_probe.py", shapes=rows), indent=1) + "\n")):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
