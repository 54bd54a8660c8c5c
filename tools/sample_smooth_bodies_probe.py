#!/usr/bin/env python3
"""Smooth sampling at the points of rigid bodies (sample_smooth_bodies_ / sample_smooth_bodies_pullback_) on one
MI355X, fp32.

    python tools/sample_smooth_bodies_probe.py [--reps 9] [--out profiles/sample_smooth_bodies_probe.txt]
                                               [--grids 512^2,128^2,128^3] [--orders sorted,shuffled] [--append]
                                               [--note TEXT]

One run; give every grid a run of its own under `timeout` (--grids, --append) so that no step can outlive its limit.
For every (grid, P, B) of SHAPES and K in KS, a uniform cloud whose bodies are contiguous runs of P / K points
("sorted") and the same cloud under a random permutation ("shuffled"):

  fwd                     sample_smooth_bodies_ (DPR_ALGO_ATOMIC, the only forward)
  pb_atomic / pb_tiled    sample_smooth_bodies_pullback_ with all four gradients on either algorithm
  pb_geom                 the same without "image" (need = points, rotation, translation): the point kernel alone, the
                          figure that decides on the LDS table of pose sums
  loop / loop_pb          the composite the op replaces: K calls of sample_smooth_ / sample_smooth_pullback_ on AUTO on
                          the subsets body == k (gathered beforehand, outside the timing); the pullback writes
                          per-subset buffers and the K - 1 image additions are not timed
  splat_pb                raster_pullback_smooth_bodies_ of the same shape and order: the same gathers and the same
                          per-(image, body) sums through the walk with global atomics

Inputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one
call (ms) after a warm-up call of every variant; the variants of a row are timed in turn within each repetition
(timed_in_turn of tools/smooth_clouds_probe.py), so that drift hits them alike.  `spread` is (max - min) / median over
the repetitions, the largest among the four fused calls."""
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
from smooth_clouds_probe import timed_in_turn, ws  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("512^2", (512, 512), 1_000_000, 16), ("128^2", (128, 128), 100_000, 64),
          ("128^3", (128, 128, 128), 1_000_000, 4)]
KS = (1, 4, 16, 64)
FUSED = ("fwd", "pb_atomic", "pb_tiled", "pb_geom")
GEOM = ("points", "rotation", "translation")


def query(grid, P, B, K, n_in):
    """dpr_workspace_bytes_sample_smooth_bodies_ex_f32 for the tiled pullback (the family has no public query)."""
    a = np.asarray(grid, dtype=np.int64)
    return int(dpr_amd.lib().dpr_workspace_bytes_sample_smooth_bodies_ex_f32(
        _lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, len(grid), a.ctypes.data_as(ctypes.c_void_p), P, B, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_smooth_bodies_probe.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--grids", default="512^2,128^2,128^3")
    ap.add_argument("--orders", default="sorted,shuffled")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    lines = []
    if not args.append:
        lines += [f"# tools/sample_smooth_bodies_probe.py: median of {args.reps} calls after a warm-up (ms), one MI355X, "
                  "fp32; P points uniform in [-1, 1)^3, K bodies of P / K points, contiguous (sorted) or under a random "
                  "permutation (shuffled)",
                  "# fwd: sample_smooth_bodies_; pb_atomic / pb_tiled: sample_smooth_bodies_pullback_, four gradients; "
                  "pb_geom: without ds_dimage; loop / loop_pb: K subset calls of sample_smooth_ / "
                  "sample_smooth_pullback_ (AUTO); splat_pb: raster_pullback_smooth_bodies_; spread: (max - min) / median "
                  "of the four fused calls, the largest; AUTO: the pullback's algorithm"]
    if args.note:
        lines.append(f"# {args.note}")
    lines.append(f"{'grid':<7}{'P':>9}{'B':>4}{'K':>4} {'order':<9}{'fwd':>8}{'pb_atomic':>10}{'pb_tiled':>9}{'pb_geom':>9}"
                 f"{'loop':>9}{'loop_pb':>9}{'splat_pb':>9}{'spread':>8}  {'AUTO':<7}{'loop/fwd':>9}{'loop_pb/AUTO':>13}"
                 f"{'other/AUTO':>11}")
    print("\n".join(lines), flush=True)
    for gname, grid, P, B in SHAPES:
        if gname not in args.grids.split(","):
            continue
        n_out = len(grid)
        for K in (int(k) for k in args.ks.split(",")):
            g = torch.Generator(device=dev).manual_seed(P % 9973 + B + K)
            pts0 = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
            body0 = (torch.arange(P, device=dev) * K // P).to(torch.int32)
            d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B * K, grid_n=grid, seed=1)
            rot = torch.as_tensor(d.rotations, dtype=dt, device=dev).reshape(B, K, n_out, n_in)
            tr = torch.as_tensor(d.translations, dtype=dt, device=dev).reshape(B, K, n_out)
            image = dpr_amd.empty_grid(grid, B, dt, dev)
            image.copy_(torch.randn(image.shape, generator=g, device=dev, dtype=dt))
            dv0 = torch.randn((B, P), generator=g, device=dev, dtype=dt)
            values = torch.empty((B, P), device=dev, dtype=dt).t()
            e = lambda *s: torch.empty(s, device=dev, dtype=dt)
            outs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, dt, dev), ds_dpoints=e(P, n_in),
                        ds_drotation=e(B, K, n_in, n_out).transpose(-1, -2), ds_dtranslation=e(B, K, n_out))
            geom = {k: v for k, v in outs.items() if k != "ds_dimage"}
            splat = dict(ds_dpoints=e(P, n_in), ds_drotation=e(B, K, n_in, n_out).transpose(-1, -2),
                         ds_dtranslation=e(B, K, n_out), ds_dbackground=e(B), ds_dout_weight=e(B), ds_dpoint_weight=e(P))
            wt = ws(query(grid, P, B, K, n_in), dev)
            for order in args.orders.split(","):
                if order == "shuffled":
                    perm = torch.randperm(P, generator=g, device=dev)
                    pts, body, dv = pts0[perm].contiguous(), body0[perm].contiguous(), dv0[:, perm].contiguous().t()
                else:
                    pts, body, dv = pts0, body0, dv0.t()
                subsets = [torch.nonzero(body == k).flatten() for k in range(K)]
                sub = [(pts[i].contiguous(), dv.t()[:, i].contiguous().t(), torch.empty((B, len(i)), device=dev).t())
                       for i in subsets]
                rk = [rot[:, k].contiguous() for k in range(K)]
                tk = [tr[:, k].contiguous() for k in range(K)]
                wl = ws(max(dpr_amd.workspace_bytes_sample_smooth("pullback", grid, len(i), B, n_in, dt)
                            for i in subsets), dev)

                def loop_fwd():
                    for k in range(K):
                        dpr_amd.sample_smooth_(sub[k][2], image, sub[k][0], rk[k], tk[k])

                def loop_pb():
                    for k in range(K):
                        dpr_amd.sample_smooth_pullback_(sub[k][1], image, sub[k][0], rk[k], tk[k], workspace=wl)

                pull = lambda **kw: dpr_amd.sample_smooth_bodies_pullback_(dv, image, pts, body, rot, tr, **kw)
                fns = {
                    "fwd": lambda: dpr_amd.sample_smooth_bodies_(values, image, pts, body, rot, tr),
                    "pb_atomic": lambda: pull(algo="atomic", **outs),
                    "pb_tiled": lambda: pull(algo="tiled", workspace=wt, **outs),
                    "pb_geom": lambda: pull(algo="atomic", need=GEOM, **geom),
                    "loop": loop_fwd, "loop_pb": loop_pb,
                    "splat_pb": lambda: dpr_amd.raster_pullback_smooth_bodies_(image, pts, body, rot, tr, **splat),
                }
                ts = timed_in_turn(fns, args.reps)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in FUSED)
                auto = dpr_amd.resolve_algo_sample_smooth_bodies("pullback", grid, P, B, K, n_in)
                other = "pb_atomic" if auto == "tiled" else "pb_tiled"
                lines.append(f"{gname:<7}{P:>9}{B:>4}{K:>4} {order:<9}{med['fwd']:8.3f}{med['pb_atomic']:10.3f}"
                             f"{med['pb_tiled']:9.3f}{med['pb_geom']:9.3f}{med['loop']:9.3f}{med['loop_pb']:9.3f}"
                             f"{med['splat_pb']:9.3f}{spread:8.2f}  {auto:<7}{med['loop'] / med['fwd']:9.2f}"
                             f"{med['loop_pb'] / med['pb_' + auto]:13.2f}{med[other] / med['pb_' + auto]:11.2f}")
                print(lines[-1], flush=True)
                del sub, subsets, wl
            del pts0, image, dv0, values, outs, geom, splat, wt
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
