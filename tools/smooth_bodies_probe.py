#!/usr/bin/env python3
"""The smooth splat of rigid bodies (raster_smooth_bodies_ / raster_pullback_smooth_bodies_) on one MI355X, fp32.

    python tools/smooth_bodies_probe.py [--reps 9] [--out profiles/smooth_bodies_probe.txt] [--json FILE]
                                        [--set main|threshold] [--append]

For every (grid, P, B) of SHAPES and K in KS, a uniform cloud whose bodies are contiguous runs of P / K points
("sorted") and the same cloud under a random permutation ("shuffled"):

  atomic / tiled / tiled_g1   raster_smooth_bodies_ on DPR_ALGO_ATOMIC, on DPR_ALGO_TILED with the default group of
                              images and with max_pose_group=1 (image by image)
  pullback                    raster_pullback_smooth_bodies_ (DPR_ALGO_ATOMIC)
  loop / loop_pb              the composite the op replaces: K calls of raster_smooth_ / raster_pullback_smooth_ on
                              AUTO on the subsets body == k (gathered beforehand, outside the timing) and the K - 1
                              image additions; the pullback writes per-subset buffers
  warp / warp_pb              the other composite: the points warped per image in torch (a gather of the per-point
                              poses and a batched matrix product, (B, P, N_out) out), raster_smooth_clouds_ /
                              raster_pullback_smooth_clouds_ on AUTO under the identity pose, and for the pullback
                              torch's backward through the warp to points, rotation, translation

Inputs are resident on the device, workspaces allocated once.  Times: median over `--reps` of HIP events around one
call (ms) after a warm-up call of every variant; the variants of a row are timed in turn within each repetition
(timed_in_turn of tools/smooth_clouds_probe.py), so that drift hits them alike.  `spread` is (max - min) / median over
the repetitions, the largest among the three fused forwards and the fused pullback.  `--json`: the same rows as a list
of dicts (the source of tests/golden/smooth_bodies_auto.json)."""
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
KS = (1, 4, 16, 64)
# --set threshold: small calls on both sides of the AUTO rule (K = 4 only), the shapes tools/smooth_clouds_probe.py
# has around the same constants
THRESHOLD = ([("128^2", (128, 128), P, B) for P, B in ((10_000, 16), (10_000, 32), (30_000, 16), (10_000, 64))]
             + [("512^2", (512, 512), 30_000, 16)]
             + [("128^3", (128,) * 3, P, B) for P, B in ((10_000, 4), (30_000, 4), (10_000, 16))]
             + [("256^3", (256,) * 3, P, B) for P, B in ((10_000, 16), (30_000, 4), (100_000, 4))])
FUSED = ("atomic", "tiled", "tiled_g1", "pullback")


def query(grid, P, B, K, n_in, max_pose_group=0):
    """dpr_workspace_bytes_smooth_bodies_ex_f32 for the tiled forward (the family has no public query)."""
    a = np.asarray(grid, dtype=np.int64)
    return int(dpr_amd.lib().dpr_workspace_bytes_smooth_bodies_ex_f32(
        _lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(max_pose_group), n_in, len(grid),
        a.ctypes.data_as(ctypes.c_void_p), P, B, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bodies_probe.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--set", default="main", choices=["main", "threshold"])
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--grids", default="512^2,128^2,128^3,256^3")
    ap.add_argument("--orders", default="sorted,shuffled")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    label = "" if args.set == "main" else f" --set {args.set}"
    lines = [f"# tools/smooth_bodies_probe.py{label}: median of {args.reps} calls after a warm-up (ms), one MI355X, fp32; P "
             "points uniform in [-1, 1)^3, point weights uniform [0.5, 1.5), K bodies of P / K points, contiguous "
             "(sorted) or under a random permutation (shuffled)",
             "# atomic / tiled / tiled_g1: raster_smooth_bodies_ (tiled_g1: max_pose_group=1); pullback: "
             "raster_pullback_smooth_bodies_; loop / loop_pb: K subset calls of raster_smooth_ / "
             "raster_pullback_smooth_ (AUTO); warp / warp_pb: torch warp + raster_smooth_clouds_ / "
             "raster_pullback_smooth_clouds_ (AUTO) + torch backward; group: images binned together by default; "
             "spread: (max - min) / median of the four fused calls, the largest",
             f"{'grid':<7}{'P':>9}{'B':>4}{'K':>4} {'order':<9}{'group':>6}{'atomic':>9}{'tiled':>9}{'tiled_g1':>9}"
             f"{'loop':>9}{'warp':>9}{'pullback':>10}{'loop_pb':>9}{'warp_pb':>9}{'spread':>8}  {'AUTO':<7}"
             f"{'best other/AUTO':>16}{'pb':>6}"]
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
            pts0 = 2 * torch.rand((P, n_in), generator=g, device=dev, dtype=dt) - 1
            pw0 = 0.5 + torch.rand((P,), generator=g, device=dev, dtype=dt)
            body0 = (torch.arange(P, device=dev) * K // P).to(torch.int32)
            d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B * K, grid_n=grid, seed=1)
            rot = torch.as_tensor(d.rotations, dtype=dt, device=dev).reshape(B, K, n_out, n_in)
            tr = torch.as_tensor(d.translations, dtype=dt, device=dev).reshape(B, K, n_out)
            bg = torch.arange(1, B + 1, dtype=dt, device=dev)
            ow = 1 + 9 * torch.rand((B,), generator=g, device=dev, dtype=dt)
            out = dpr_amd.empty_grid(grid, B, dt, dev)
            tmp = dpr_amd.empty_grid(grid, B, dt, dev)
            ds = dpr_amd.empty_grid(grid, B, dt, dev)
            ds.copy_(torch.randn(ds.shape, generator=g, device=dev, dtype=dt))
            eye = torch.eye(n_out, dtype=dt, device=dev).expand(B, n_out, n_out).contiguous()
            zero_t = torch.zeros((B, n_out), dtype=dt, device=dev)
            wt, w1 = ws(query(grid, P, B, K, n_in), dev), ws(query(grid, P, B, K, n_in, 1), dev)
            wc = ws(dpr_amd.workspace_bytes_smooth_clouds("raster", grid, P, B, n_out, dt), dev)
            for order in args.orders.split(","):
                if order == "shuffled":
                    perm = torch.randperm(P, generator=g, device=dev)
                    pts, pw, body = pts0[perm].contiguous(), pw0[perm].contiguous(), body0[perm].contiguous()
                else:
                    pts, pw, body = pts0, pw0, body0
                body64 = body.long()
                subsets = [torch.nonzero(body == k).flatten() for k in range(K)]
                sub = [(pts[i].contiguous(), pw[i].contiguous()) for i in subsets]
                rk = [rot[:, k].contiguous() for k in range(K)]
                tk = [tr[:, k].contiguous() for k in range(K)]
                wl = ws(max(dpr_amd.workspace_bytes_smooth("raster", grid, len(i), B, n_in, dt) for i in subsets), dev)

                def warp(p, R, t):  # (B, P, N_out): every point under the pose of its body in every image
                    return torch.einsum("bpij,pj->bpi", R[:, body64], p) + t[:, body64]

                def warp_fwd():
                    dpr_amd.raster_smooth_clouds_(out, warp(pts, rot, tr), eye, zero_t, bg, ow, pw, workspace=wc)

                def warp_pb():
                    p, R, t = (x.detach().requires_grad_() for x in (pts, rot, tr))
                    w = warp(p, R, t)
                    pb = dpr_amd.raster_pullback_smooth_clouds_(ds, w.detach(), eye, zero_t, bg, ow, pw)
                    w.backward(pb.points)

                def loop_fwd():
                    for k in range(K):
                        dpr_amd.raster_smooth_(out if k == 0 else tmp, sub[k][0], rk[k], tk[k], bg if k == 0 else None,
                                               ow, sub[k][1], workspace=wl)
                        if k:
                            out.add_(tmp)

                def loop_pb():
                    for k in range(K):
                        dpr_amd.raster_pullback_smooth_(ds, sub[k][0], rk[k], tk[k], None, ow, sub[k][1])

                fused = lambda **kw: dpr_amd.raster_smooth_bodies_(out, pts, body, rot, tr, bg, ow, pw, **kw)
                fns = {
                    "atomic": lambda: fused(algo="atomic"),
                    "tiled": lambda: fused(algo="tiled", workspace=wt),
                    "tiled_g1": lambda: fused(algo="tiled", workspace=w1, max_pose_group=1),
                    "loop": loop_fwd, "warp": warp_fwd,
                    "pullback": lambda: dpr_amd.raster_pullback_smooth_bodies_(ds, pts, body, rot, tr, bg, ow, pw),
                    "loop_pb": loop_pb, "warp_pb": warp_pb,
                }
                ts = timed_in_turn(fns, args.reps)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in FUSED)
                auto = dpr_amd.resolve_algo_smooth_bodies("raster", grid, P, B, K, n_in)
                lines.append(f"{gname:<7}{P:>9}{B:>4}{K:>4} {order:<9}{group:>6}{med['atomic']:9.3f}{med['tiled']:9.3f}"
                             f"{med['tiled_g1']:9.3f}{med['loop']:9.3f}{med['warp']:9.3f}{med['pullback']:10.3f}"
                             f"{med['loop_pb']:9.3f}{med['warp_pb']:9.3f}{spread:8.2f}  {auto:<7}"
                             f"{min(med['loop'], med['warp']) / med[auto]:16.2f}"
                             f"{min(med['loop_pb'], med['warp_pb']) / med['pullback']:6.2f}")
                print(lines[-1], flush=True)
                rows.append(dict(grid=list(grid), P=P, B=B, K=K, n_in=n_in, order=order, group=group, auto=auto,
                                 spread=round(spread, 3), ms={k: round(v, 4) for k, v in med.items()}))
                del sub, subsets, wl
            del pts0, pw0, out, tmp, ds, wt, w1, wc
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
