#!/usr/bin/env python3
"""The forward mode of the smooth splat of rigid bodies (raster_smooth_bodies_jvp_) on one MI355X, fp32.

    python tools/smooth_bodies_jvp_probe.py [--reps 9] [--out profiles/smooth_bodies_jvp_probe.txt] [--json FILE]
                                            [--set main|threshold] [--append]

For every (grid, P, B) of SHAPES, K in KS and V in VS, a uniform cloud whose bodies are contiguous runs of P / K points
("sorted") and the same cloud under a random permutation ("shuffled"), all six tangents given:

  atomic / tiled / tiled_g1   raster_smooth_bodies_jvp_ on DPR_ALGO_ATOMIC, on DPR_ALGO_TILED with the default group of
                              images and with max_pose_group=1 (image by image)
  loop                        the composite the op replaces: K calls of raster_smooth_jvp_ on AUTO on the subsets
                              body == k (points and their tangents gathered beforehand, outside the timing) and the
                              K - 1 image additions
  fwd_t                       raster_smooth_bodies_ on DPR_ALGO_TILED (default group), the same shape: the yardstick
                              for one plane of `tiled`

Inputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one
call (ms) after a warm-up call of every variant; the variants of a row are timed in turn within each repetition
(timed_in_turn of tools/smooth_clouds_probe.py), so that drift hits them alike.  `spread` is (max - min) / median over
the repetitions, the largest among the three fused calls.  `--json`: the same rows as a list of dicts (the source of
tests/golden/smooth_bodies_jvp_auto.json)."""
import argparse
import ctypes
import json
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
KS = (1, 4, 64)
VS = (1, 12)
# --set threshold: small calls on both sides of the AUTO rule (K = 4 only).  With V = 12 a bound on bg * P * V is
# crossed by clouds a twelfth the size of those that cross it with V = 1; 256^3: the 4 points per tile
THRESHOLD = ([("128^2", (128, 128), P, B) for P, B in ((1_000, 4), (2_000, 4), (3_000, 4), (5_000, 4), (10_000, 1),
                                                       (10_000, 2), (10_000, 8), (10_000, 12), (10_000, 16),
                                                       (30_000, 16))]
             + [("512^2", (512, 512), 30_000, 16)]
             + [("64^3", (64,) * 3, P, B) for P, B in ((1_100, 2), (1_100, 4), (1_500, 4), (2_000, 4), (3_000, 4),
                                                       (10_000, 4), (24_000, 4), (30_000, 4))]
             + [("128^3", (128,) * 3, P, B) for P, B in ((10_000, 1), (10_000, 4), (30_000, 4), (10_000, 16))]
             + [("256^3", (256,) * 3, P, B) for P, B in ((10_000, 16), (30_000, 4), (100_000, 4))])
FUSED = ("atomic", "tiled", "tiled_g1")
NAMES = ("points_dot", "rotation_dot", "translation_dot", "background_dot", "out_weight_dot", "point_weight_dot")


def query(grid, P, B, K, V, n_in, max_pose_group=0):
    """dpr_workspace_bytes_smooth_bodies_jvp_ex_f32 for the tiled call (the family has no public query)."""
    a = np.asarray(grid, dtype=np.int64)
    return int(dpr_amd.lib().dpr_workspace_bytes_smooth_bodies_jvp_ex_f32(
        _lib.ALGO_TILED, _lib.flag_max_pose_group(max_pose_group), n_in, len(grid), a.ctypes.data_as(ctypes.c_void_p),
        P, B, K, V))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bodies_jvp_probe.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--set", default="main", choices=["main", "threshold"])
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--grids", default="512^2,128^2,64^3,128^3,256^3")
    ap.add_argument("--orders", default="sorted,shuffled")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    label = "" if args.set == "main" else f" --set {args.set}"
    lines = [f"# tools/smooth_bodies_jvp_probe.py{label}: median of {args.reps} calls after a warm-up (ms), one MI355X, "
             "fp32; P points uniform in [-1, 1)^3, point weights uniform [0.5, 1.5), K bodies of P / K points, contiguous "
             "(sorted) or under a random permutation (shuffled); V tangents ~ N(0, 1), all six given",
             "# atomic / tiled / tiled_g1: raster_smooth_bodies_jvp_ (tiled_g1: max_pose_group=1); loop: K subset calls "
             "of raster_smooth_jvp_ (AUTO) + K - 1 additions; fwd_t: raster_smooth_bodies_ tiled, the same shape; group: "
             "images binned together by default; spread: (max - min) / median of the three fused calls, the largest; "
             "t/(V fwd_t): a tiled plane against one tiled forward",
             f"{'grid':<7}{'P':>9}{'B':>4}{'K':>4}{'V':>4} {'order':<9}{'group':>6}{'atomic':>9}{'tiled':>9}{'tiled_g1':>9}"
             f"{'loop':>9}{'fwd_t':>9}{'spread':>8}  {'AUTO':<7}{'AUTO/best':>10}{'loop/AUTO':>10}{'t/(V fwd_t)':>12}"]
    print("\n".join(lines), flush=True)
    rows = []
    for gname, grid, P, B in (SHAPES if args.set == "main" else THRESHOLD):
        if gname not in args.grids.split(","):
            continue
        n_out = len(grid)
        tiles = int(np.prod([-(-n // e) for n, e in zip(grid, (64, 16) if n_out == 2 else (16, 8, 8))]))
        group = min(B, max(1, (1 << 24) // max(P, tiles)))  # (include/dpr.h, GROUP SIZE)
        for K in (KS if args.set == "main" else (4,)):
            g = torch.Generator(device=dev).manual_seed(P % 9973 + B + K)
            rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=dt)
            pts0 = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
            pw0 = 0.5 + torch.rand((P,), generator=g, device=dev, dtype=dt)
            body0 = (torch.arange(P, device=dev) * K // P).to(torch.int32)
            d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B * K, grid_n=grid, seed=1)
            rot = torch.as_tensor(d.rotations, dtype=dt, device=dev).reshape(B, K, n_out, n_in)
            tr = torch.as_tensor(d.translations, dtype=dt, device=dev).reshape(B, K, n_out)
            bg = torch.arange(1, B + 1, dtype=dt, device=dev)
            ow = 1 + 9 * torch.rand((B,), generator=g, device=dev, dtype=dt)
            fwd_out = dpr_amd.empty_grid(grid, B, dt, dev)
            w_fwd = ws(query(grid, P, B, K, 1, n_in), dev)  # (the forward's workspace is the same bytes)
            for V in VS:
                out = dpr_amd.empty_channel_grid(grid, V, B, dt, dev)
                tmp = dpr_amd.empty_channel_grid(grid, V, B, dt, dev)
                pd0, pwd0 = rnd(V, P, n_in), rnd(V, P)
                pose_t = dict(rotation_dot=rnd(V, B, K, n_out, n_in), translation_dot=rnd(V, B, K, n_out),
                              background_dot=rnd(V, B), out_weight_dot=rnd(V, B))
                wt, w1 = ws(query(grid, P, B, K, V, n_in), dev), ws(query(grid, P, B, K, V, n_in, 1), dev)
                for order in args.orders.split(","):
                    if order == "shuffled":
                        perm = torch.randperm(P, generator=g, device=dev)
                        pts, pw, body = pts0[perm].contiguous(), pw0[perm].contiguous(), body0[perm].contiguous()
                        pd, pwd = pd0[:, perm].contiguous(), pwd0[:, perm].contiguous()
                    else:
                        pts, pw, body, pd, pwd = pts0, pw0, body0, pd0, pwd0
                    tan = dict(points_dot=pd, point_weight_dot=pwd, **pose_t)
                    subsets = [torch.nonzero(body == k).flatten() for k in range(K)]
                    sub = [dict(points=pts[i].contiguous(), pw=pw[i].contiguous(), rot=rot[:, k].contiguous(),
                                trans=tr[:, k].contiguous(), points_dot=pd[:, i].contiguous(),
                                point_weight_dot=pwd[:, i].contiguous(),
                                rotation_dot=pose_t["rotation_dot"][:, :, k].contiguous(),
                                translation_dot=pose_t["translation_dot"][:, :, k].contiguous())
                           for k, i in enumerate(subsets)]
                    wl = ws(max(dpr_amd.workspace_bytes_smooth_jvp(grid, len(i), B, n_in, V, dt, algo="tiled")
                                for i in subsets), dev)

                    def loop():
                        for k, s in enumerate(sub):
                            dpr_amd.raster_smooth_jvp_(
                                out if k == 0 else tmp, s["points"], s["rot"], s["trans"], None, ow, s["pw"],
                                points_dot=s["points_dot"], rotation_dot=s["rotation_dot"],
                                translation_dot=s["translation_dot"],
                                background_dot=pose_t["background_dot"] if k == 0 else None,
                                out_weight_dot=pose_t["out_weight_dot"], point_weight_dot=s["point_weight_dot"],
                                tangents=V, workspace=wl)
                            if k:
                                out.add_(tmp)

                    fused = lambda **kw: dpr_amd.raster_smooth_bodies_jvp_(out, pts, body, rot, tr, bg, ow, pw, **tan,
                                                                           tangents=V, **kw)
                    fns = {
                        "atomic": lambda: fused(algo="atomic"),
                        "tiled": lambda: fused(algo="tiled", workspace=wt),
                        "tiled_g1": lambda: fused(algo="tiled", workspace=w1, max_pose_group=1),
                        "loop": loop,
                        "fwd_t": lambda: dpr_amd.raster_smooth_bodies_(fwd_out, pts, body, rot, tr, bg, ow, pw,
                                                                       algo="tiled", workspace=w_fwd),
                    }
                    ts = timed_in_turn(fns, args.reps)
                    med = {k: float(np.median(v)) for k, v in ts.items()}
                    spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in FUSED)
                    auto = dpr_amd.resolve_algo_smooth_bodies_jvp(grid, P, B, K, n_in, V)
                    best = min(med["atomic"], med["tiled"])
                    lines.append(f"{gname:<7}{P:>9}{B:>4}{K:>4}{V:>4} {order:<9}{group:>6}{med['atomic']:9.3f}"
                                 f"{med['tiled']:9.3f}{med['tiled_g1']:9.3f}{med['loop']:9.3f}{med['fwd_t']:9.3f}"
                                 f"{spread:8.2f}  {auto:<7}{med[auto] / best:10.2f}{med['loop'] / med[auto]:10.2f}"
                                 f"{med['tiled'] / (V * med['fwd_t']):12.2f}")
                    print(lines[-1], flush=True)
                    rows.append(dict(grid=list(grid), P=P, B=B, K=K, V=V, n_in=n_in, order=order, group=group,
                                     auto=auto, spread=round(spread, 3), ms={k: round(v, 4) for k, v in med.items()}))
                    del sub, subsets, wl
                del out, tmp, pd0, pwd0, wt, w1
            del pts0, pw0, fwd_out, w_fwd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
