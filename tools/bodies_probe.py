#!/usr/bin/env python3
"""The rigid-body op (raster_bodies_ / raster_pullback_bodies_) on one MI355X, fp32.

    python tools/bodies_probe.py [--reps 9] [--out profiles/bodies_probe.txt] [--json FILE]
                                 [--fused-only] [--append] [--label TEXT]

For every (grid, P, B) of SHAPES and K in KS, a uniform cloud whose bodies are contiguous runs of P / K points
("sorted") and the same cloud under a random permutation ("shuffled"), forward and pullback:

  fused     raster_bodies_ / raster_pullback_bodies_
  raster    raster_ / raster_pullback_ on DPR_ALGO_ATOMIC for the same P and B under the poses of body 0: the K = 1
            floor, what the per-body indirection and the segmented sums cost over the core kernels
  warp      the composite the op replaces: the points warped per image in torch (a gather of the per-point poses and
            a batched matrix product, (B, P, N_out) out), raster_clouds_ / raster_pullback_clouds_ on AUTO under the
            identity pose, and for the pullback torch's backward through the warp to points, rotation, translation
  loop      the other composite: K calls of raster_ / raster_pullback_ on AUTO on the subsets body == k (gathered
            beforehand, outside the timing) and the K - 1 image additions; the pullback writes per-subset buffers

Inputs are resident on the device.  Times: median over `--reps` of HIP events around one call (ms) after a warm-up
call of every variant; the variants of a row are timed in turn within each repetition (timed_in_turn of
tools/smooth_clouds_probe.py), so that drift hits them alike.  `spread` is (max - min) / median over the repetitions,
the larger of the two fused calls.  `bodies/wave`: mean number of distinct bodies among 64 consecutive points.
`--fused-only` times the fused calls alone (for a library built another way, loaded through DPR_LIB_OVERRIDE);
`--append --label` add such a run to the file as a section of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dpr_amd  # noqa: E402
from smooth_clouds_probe import timed_in_turn  # noqa: E402
from tests import data as D  # noqa: E402

SHAPES = [("128^2", (128, 128), 100_000, 64), ("512^2", (512, 512), 1_000_000, 16),
          ("128^3", (128, 128, 128), 1_000_000, 4)]
KS = (1, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies_probe.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--orders", default="sorted,shuffled")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt, n_in = torch.float32, 3
    head = [f"# tools/bodies_probe.py{' ' + args.label if args.label else ''}: median of {args.reps} calls after a "
            "warm-up (ms), one MI355X, fp32; P points uniform in [-1, 1)^3, point weights uniform [0.5, 1.5), K bodies "
            "of P / K points, contiguous (sorted) or under a random permutation (shuffled)",
            "# fused: raster_bodies_ / raster_pullback_bodies_; raster: raster_ / raster_pullback_ (ATOMIC), one pose "
            "per image; warp: torch warp + raster_clouds_ / raster_pullback_clouds_ + torch backward; loop: K subset "
            "calls of raster_ / raster_pullback_ (AUTO); spread: (max - min) / median of the fused calls, the larger",
            f"{'grid':<7}{'P':>9}{'B':>4}{'K':>4} {'order':<9}{'bodies/wave':>12}{'fused':>9}{'raster':>9}{'warp':>9}"
            f"{'loop':>9}{'fused_pb':>10}{'raster_pb':>10}{'warp_pb':>9}{'loop_pb':>9}{'spread':>8}"
            f"{'fused/raster':>13}{'pb':>6}{'best other/fused':>17}{'pb':>6}"]
    lines, rows = list(head), []
    print("\n".join(head), flush=True)
    for gname, grid, P, B in SHAPES:
        n_out = len(grid)
        for K in KS:
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
            for order in args.orders.split(","):
                if order == "shuffled":
                    perm = torch.randperm(P, generator=g, device=dev)
                    pts, pw, body = pts0[perm].contiguous(), pw0[perm].contiguous(), body0[perm].contiguous()
                else:
                    pts, pw, body = pts0, pw0, body0
                per_wave = float(np.mean([len(np.unique(w)) for w in
                                          body[:64 * min(P // 64, 2000)].cpu().numpy().reshape(-1, 64)]))
                body64 = body.long()
                subsets = [torch.nonzero(body == k).flatten() for k in range(K)]
                sub = [(pts[i].contiguous(), pw[i].contiguous()) for i in subsets]
                r0, t0 = rot[:, 0].contiguous(), tr[:, 0].contiguous()
                rk = [rot[:, k].contiguous() for k in range(K)]
                tk = [tr[:, k].contiguous() for k in range(K)]
                ws_sub = [dpr_amd.workspace_bytes("raster", grid, len(i), B, n_in, dt) for i in subsets]
                ws_sub += [dpr_amd.workspace_bytes("pullback", grid, len(i), B, n_in, dt) for i in subsets]
                wl = torch.empty(max(max(ws_sub), 256), dtype=torch.uint8, device=dev)
                wc = torch.empty(max(dpr_amd.workspace_bytes_clouds("raster", grid, P, B, n_out, dt),
                                     dpr_amd.workspace_bytes_clouds("pullback", grid, P, B, n_out, dt), 256),
                                 dtype=torch.uint8, device=dev)

                def warp(p, R, t):  # (B, P, N_out): every point under the pose of its body in every image
                    return torch.einsum("bpij,pj->bpi", R[:, body64], p) + t[:, body64]

                def warp_fwd():
                    dpr_amd.raster_clouds_(out, warp(pts, rot, tr), eye, zero_t, bg, ow, pw, workspace=wc)

                def warp_pb():
                    p, R, t = (x.detach().requires_grad_() for x in (pts, rot, tr))
                    w = warp(p, R, t)
                    pb = dpr_amd.raster_pullback_clouds_(ds, w.detach(), eye, zero_t, bg, ow, pw, workspace=wc)
                    w.backward(pb.points)

                def loop_fwd():
                    for k in range(K):
                        dpr_amd.raster_(out if k == 0 else tmp, sub[k][0], rk[k], tk[k], bg if k == 0 else None, ow,
                                        sub[k][1], workspace=wl)
                        if k:
                            out.add_(tmp)

                def loop_pb():
                    for k in range(K):
                        dpr_amd.raster_pullback_(ds, sub[k][0], rk[k], tk[k], None, ow, sub[k][1], workspace=wl)

                fns = {
                    "fused": lambda: dpr_amd.raster_bodies_(out, pts, body, rot, tr, bg, ow, pw),
                    "fused_pb": lambda: dpr_amd.raster_pullback_bodies_(ds, pts, body, rot, tr, bg, ow, pw),
                }
                if not args.fused_only:
                    fns.update({
                        "raster": lambda: dpr_amd.raster_(out, pts, r0, t0, bg, ow, pw, algo="atomic"),
                        "raster_pb": lambda: dpr_amd.raster_pullback_(ds, pts, r0, t0, bg, ow, pw, algo="atomic"),
                        "warp": warp_fwd, "warp_pb": warp_pb, "loop": loop_fwd, "loop_pb": loop_pb,
                    })
                ts = timed_in_turn(fns, args.reps)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                spread = max((max(ts[k]) - min(ts[k])) / med[k] for k in ("fused", "fused_pb"))
                col = lambda k, w: f"{med[k]:{w}.3f}" if k in med else f"{'-':>{w}}"
                ratio = lambda a, b, w: f"{med[a] / med[b]:{w}.2f}" if a in med and b in med else f"{'-':>{w}}"
                best = lambda suf, w: (f"{min(med['warp' + suf], med['loop' + suf]) / med['fused' + suf]:{w}.2f}"
                                       if "warp" in med else f"{'-':>{w}}")
                lines.append(f"{gname:<7}{P:>9}{B:>4}{K:>4} {order:<9}{per_wave:>12.1f}{col('fused', 9)}"
                             f"{col('raster', 9)}{col('warp', 9)}{col('loop', 9)}{col('fused_pb', 10)}"
                             f"{col('raster_pb', 10)}{col('warp_pb', 9)}{col('loop_pb', 9)}{spread:8.2f}"
                             f"{ratio('fused', 'raster', 13)}{ratio('fused_pb', 'raster_pb', 6)}{best('', 17)}"
                             f"{best('_pb', 6)}")
                print(lines[-1], flush=True)
                rows.append(dict(grid=list(grid), P=P, B=B, K=K, order=order, bodies_per_wave=round(per_wave, 2),
                                 spread=round(spread, 3), label=args.label, ms={k: round(v, 4) for k, v in med.items()}))
                del sub, subsets, wl, wc
            del pts0, pw0, out, tmp, ds
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
