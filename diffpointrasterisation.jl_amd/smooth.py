"""The smooth splat: `raster` with quadratic B-spline weights on 3^N cells per point, forward and pullback
(dpr_raster_smooth_ex_* / dpr_raster_pullback_smooth_ex_*, include/dpr.h "SMOOTH SPLAT").

`raster` deposits a point with N-linear weights on 2^N cells; its gradient jumps whenever a point crosses a cell
boundary.  `raster_smooth` deposits with the next kernel order up (particle-in-cell codes: TSC): the weights are
C1 in the point position and sum to 1, so the pullback is continuous and agrees with finite differences
everywhere.  For axis d with n_d cells:

    coord_d = ((R p + t)_d + 1) * n_d / 2,  j0_d = floor(coord_d),  u_d = coord_d - (j0_d + 1/2)
    w_d(-1) = (1/2 - u_d)^2 / 2     w_d(0) = 3/4 - u_d^2     w_d(+1) = (1/2 + u_d)^2 / 2
    out[j0 + s, b] += out_weight[b] * point_weight[p] * prod_d w_d(s_d),   s in {-1, 0, +1}^N_out

Argument shapes, layouts, batching (single pose or batch), defaults, `background`, `out_weight` and `point_weight`
are those of `raster` / `raster_pullback_`.  (N_in, N_out): (2,2), (3,3), (3,2).  Algorithms: "atomic" (forward and
pullback), "tiled" (forward), "auto".
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (ColumnMajorRotation, DimensionMismatch, _alloc_like, _canonicalise, _cast_grads, _check_dims,
                    _detach, _image, _launch, _op_code, _out_buf, _per_pose, _resolve, _restore, _rotation_buf,
                    _save, _workspace_bytes, empty_grid)
from .interface import PullbackResult

_ACCEPTED_OPS = ("raster", "pullback")
_PAIRS = ((2, 2), (3, 3), (3, 2))


def resolve_algo_smooth(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth call (dpr_resolve_algo_smooth); op is "raster" or
    "pullback"."""
    return _resolve("dpr_resolve_algo_smooth", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch, n_in)


def workspace_bytes_smooth(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                           algo: str = "auto") -> int:
    """dpr_workspace_bytes_smooth_ex_*: device bytes a smooth call needs."""
    return _workspace_bytes("_smooth", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in)


def _check_shapes(points, rotation, translation):
    """The dimension errors of a smooth call, raised before anything else looks at the arguments (and before any
    library call): the funnel's own, and the (N_in, N_out) pairs the smooth splat has."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor on a HIP device")
    if points.ndim != 2:
        raise DimensionMismatch(f"points must be (P, N_in), got {tuple(points.shape)}")
    rs = tuple(rotation.shape) if isinstance(rotation, (torch.Tensor, ColumnMajorRotation)) \
        else tuple(torch.as_tensor(rotation).shape)
    ts = tuple(translation.shape) if isinstance(translation, torch.Tensor) else tuple(torch.as_tensor(translation).shape)
    if len(rs) not in (2, 3):
        raise DimensionMismatch("rotation must be (N_out, N_in) or (B, N_out, N_in)")
    if len(ts) != len(rs) - 1:
        raise DimensionMismatch(f"translation {ts} does not go with rotation {rs}")
    _check_dims(points.shape[1], rs, ts)
    if len(rs) == 3 and ts[0] != rs[0]:
        raise DimensionMismatch(f"batch sizes differ: rotation {rs[0]}, translation {ts[0]}")
    if (rs[-1], rs[-2]) not in _PAIRS:
        raise DimensionMismatch(f"raster_smooth supports (N_in, N_out) in {_PAIRS}, got {(rs[-1], rs[-2])}")


def _canonicalise_smooth(points, rotation, translation, background, out_weight, point_weight, extra=()):
    _check_shapes(points, rotation, translation)
    return _canonicalise(points, rotation, translation, background, out_weight, point_weight, extra=extra)


def raster_smooth(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                  *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward.  Returns `out[i_1..i_N]` for a single pose (rotation is a matrix) or
    `out[i_1..i_N, b]` for a batch."""
    _check_shapes(points, rotation, translation)
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), batch, dtype, device)
    return raster_smooth_(out, points, rotation, translation, background, out_weight, point_weight, algo=algo,
                          workspace=workspace)


def raster_smooth_(out, points, rotation, translation, background=None, out_weight=None, point_weight=None, *,
                   algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place forward: `out` (memory order of `empty_grid`) is fully overwritten and returned.  Enqueued on
    torch's current stream; not synchronised."""
    c = _canonicalise_smooth(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    _launch("_smooth", "dpr_raster_smooth_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, 0, workspace,
            out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    return out


def raster_pullback_smooth_(ds_dout, points, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                            ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None, algo: str = "auto",
                            workspace=None, point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_smooth`: the exact derivative (the operator is C1).  Keyword outputs are pre-allocated
    buffers, OVERWRITTEN and returned by identity, with the shapes of `raster_pullback_`; a single pose gets
    unbatched results.  `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither
    allocated nor written and comes back as None."""
    c = _canonicalise_smooth(points, rotation, translation, background, out_weight, point_weight, extra=(ds_dout,))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    g = _image(ds_dout, "ds_dout", c)
    d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    # (a single pose hands in unbatched buffers; a batch's are used, and returned, as they are)
    d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=c["single"])
    d_bg = _out_buf(ds_dbackground, (B,), "ds_dbackground", c, reshape=c["single"])
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c, reshape=c["single"])
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = _out_buf(ds_dpoint_weight, (P,), "ds_dpoint_weight", c) if point_weight_grad else None
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    _launch("_smooth", "dpr_raster_pullback_smooth_ex", _lib.OP_PULLBACK, c, g.shape[:n_out], algo, flags,
            workspace, g, c["points"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg, d_ow,
            d_pw)
    rot, trans, bg, ow = _per_pose(c, d_rot, d_trans, d_bg, d_ow)
    return PullbackResult(d_pts, rot, trans, bg, ow, d_pw)


class _RasterSmoothFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, background, out_weight, point_weight):
        out = raster_smooth(grid_size, _detach(points), _detach(rotation), _detach(translation),
                            _detach(background), _detach(out_weight), _detach(point_weight), algo=algo)
        saved = _save(ctx, (points, rotation, translation), (background, out_weight, point_weight))
        ctx.save_for_forward(*saved)
        ctx.grid_size, ctx.caller_algo = tuple(int(n) for n in grid_size), algo
        # the pullback has DPR_ALGO_ATOMIC only: a forward on "tiled" differentiates on "auto"
        ctx.algo = "auto" if algo == "tiled" else algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation), opt = _restore(ctx, 3)
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_smooth_(ds_dout.detach(), _detach(points), _detach(rotation), _detach(translation),
                                     *map(_detach, opt), algo=ctx.algo,
                                     point_weight_grad=bool(ctx.opt_is_tensor[2] and need[7]))
        return (None, None, *_cast_grads(need[2:], pb, (points, rotation, translation, *opt)))

    @staticmethod
    def jvp(ctx, _grid_t, _algo_t, points_t, rotation_t, translation_t, background_t, out_weight_t, point_weight_t):
        from .smooth_jvp import raster_smooth_jvp  # (smooth_jvp imports this module)

        (points, rotation, translation), opt = _restore(ctx, 3)
        algo = ctx.caller_algo if ctx.caller_algo in ("atomic", "tiled") else "auto"
        return raster_smooth_jvp(ctx.grid_size, _detach(points), _detach(rotation), _detach(translation),
                                 *map(_detach, opt), points_dot=points_t, rotation_dot=rotation_t,
                                 translation_dot=translation_t, background_dot=background_t,
                                 out_weight_dot=out_weight_t, point_weight_dot=point_weight_t, algo=algo)


def raster_smooth_ad(grid_size, points, rotation, translation, background=None, out_weight=None,
                     point_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_smooth` (torch autograd) in points, rotation, translation, background, out_weight
    and point_weight (whichever are tensors that require grad); the tangents are those of
    `raster_pullback_smooth_`.  Forward mode (torch.autograd.forward_ad dual tensors, torch.func.jvp) goes through
    `raster_smooth_jvp` with one tangent, on the caller's algorithm ("atomic" / "tiled") or AUTO."""
    return _RasterSmoothFn.apply(tuple(grid_size), algo, points, rotation, translation, background, out_weight,
                                 point_weight)
