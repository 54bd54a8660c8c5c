"""The smooth splat with C weights per point: `raster_smooth` into (grid..., C[, B]) images, forward and pullback
(dpr_raster_smooth_channels_ex_* / dpr_raster_pullback_smooth_channels_ex_*, include/dpr.h "SMOOTH SPLAT,
MULTI-CHANNEL").

For channel c and pose b

    out[i.., c, b] = background[b, c] + out_weight[b] * sum_p point_weight[p, c] * prod_d w_d(i_d; R_b p + t_b)

with the quadratic B-spline weights w_d, the cell choice and the acceptance rule of `raster_smooth`: plane c is
`raster_smooth(..., background=background[..., c], point_weight=point_weight[:, c])`.  The cell, the weights and the
offsets of a (point, pose) are computed once for the C channels.  Shapes and memory are those of `raster_channels`:

  point_weight  (P, C)                       a point's C weights contiguous
  background    (C,) single pose, (B, C)
  out, ds_dout  grid_size + (C,) [+ (B,)]    memory of a contiguous (B, C, n_N, .., n_1) tensor:
                                             `empty_channel_grid` allocates it

out_weight is one scalar per pose, shared by the channels.  The pullback is the exact derivative (the operator is
C1): ds_dpoints / rotation / translation / out_weight are sums over the channels, point_weight (P, C) and background
(C,) / (B, C) are per channel.  (N_in, N_out): (2,2), (3,3), (3,2); C = 1..16.  Algorithms: "atomic" (forward and
pullback), "tiled" (forward), "auto".
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (ColumnMajorRotation, DimensionMismatch, _alloc_like, _cast_grads, _detach, _image, _launch, _op_code, _out_buf,
                    _per_pose, _resolve, _restore, _rotation_buf, _save, _workspace_bytes)
from .channels import _canonicalise_channels, _check_channels, _infer_channels, empty_channel_grid
from .interface import PullbackResult
from .smooth import _check_shapes

_ACCEPTED_OPS = ("raster", "pullback")


def resolve_algo_smooth_channels(op: str, grid_size, n_points: int, batch: int, n_in: int, channels: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth channel call (dpr_resolve_algo_smooth_channels); op
    is "raster" or "pullback"."""
    return _resolve("dpr_resolve_algo_smooth_channels", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch,
                    n_in, channels)


def workspace_bytes_smooth_channels(op: str, grid_size, n_points: int, batch: int, n_in: int, channels: int,
                                    dtype=torch.float32, algo: str = "auto") -> int:
    """dpr_workspace_bytes_smooth_channels_ex_*: device bytes a smooth channel call needs."""
    return _workspace_bytes("_smooth_channels", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in, channels)


def _shape(x):
    return tuple(x.shape) if isinstance(x, (torch.Tensor, ColumnMajorRotation)) else tuple(torch.as_tensor(x).shape)


def _check_channel_shapes(points, rotation, translation, point_weight, background):
    """The dimension errors of a smooth channel call, raised before anything else looks at the arguments (and
    before any library call): those of `raster_smooth`, then point_weight (P, C) with C in 1..16 and background
    (C,) / (B, C).  `_canonicalise_channels` makes the last two checks as well, but only after it has asked for
    the device of `points`; these come first so that a wrong shape is a DimensionMismatch wherever the tensors live."""
    _check_shapes(points, rotation, translation)
    if point_weight is None:
        raise DimensionMismatch("point_weight: the channel API needs a (P, C) point_weight (C = its last dim)")
    pw, P = _shape(point_weight), points.shape[0]
    if len(pw) != 2 or pw[0] != P:
        raise DimensionMismatch(f"size(point_weight) = {pw} must be (n_points = {P}, C)")
    _check_channels(pw[1])
    if background is not None:
        rs = _shape(rotation)
        want = (pw[1],) if len(rs) == 2 else (rs[0], pw[1])
        if _shape(background) != want:
            raise DimensionMismatch(f"size(background) = {_shape(background)} must be {want}")


def _canonicalise_smooth_channels(points, rotation, translation, background, out_weight, point_weight, extra=()):
    _check_channel_shapes(points, rotation, translation, point_weight, background)
    return _canonicalise_channels(points, rotation, translation, background, out_weight, point_weight, extra=extra)


def raster_smooth_channels(grid_size, points, rotation, translation, point_weight, background=None, out_weight=None,
                           *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N, c] (single pose) or out[i_1..i_N, c, b]."""
    _check_channel_shapes(points, rotation, translation, point_weight, background)
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    C = _infer_channels(point_weight)
    out = empty_channel_grid(tuple(grid_size), C, batch, dtype, device)
    return raster_smooth_channels_(out, points, rotation, translation, point_weight, background, out_weight,
                                   algo=algo, workspace=workspace)


def raster_smooth_channels_(out, points, rotation, translation, point_weight, background=None, out_weight=None,
                            *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place forward: `out` (grid_size + (C,) [+ (B,)], `empty_channel_grid` memory order) is fully overwritten
    and returned.  Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_smooth_channels(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, (("channels", c["C"]),), out=True)
    _launch("_smooth_channels", "dpr_raster_smooth_channels_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, 0,
            workspace, out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], tail=(c["C"],))
    return out


def raster_pullback_smooth_channels_(ds_dout, points, rotation, translation, point_weight, background=None,
                                     out_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                                     ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None,
                                     algo: str = "auto", workspace=None,
                                     point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_smooth_channels`.  Keyword outputs as for `raster_pullback_channels_` (overwritten,
    returned by identity): ds_dpoint_weight (P, C), ds_dbackground (C,) / (B, C).  `point_weight_grad=False`
    (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither allocated nor written and comes back as None."""
    c = _canonicalise_smooth_channels(points, rotation, translation, background, out_weight, point_weight,
                                      extra=(ds_dout,))
    P, B, C, n_in, n_out = c["P"], c["B"], c["C"], c["n_in"], c["n_out"]
    gt = _image(ds_dout, "ds_dout", c, (("channels", C),))
    d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    # (a single pose hands in unbatched buffers; a batch's are used, and returned, as they are)
    d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=c["single"])
    d_bg = _out_buf(ds_dbackground, (B, C), "ds_dbackground", c, reshape=c["single"])
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c, reshape=c["single"])
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = _out_buf(ds_dpoint_weight, (P, C), "ds_dpoint_weight", c) if point_weight_grad else None
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    _launch("_smooth_channels", "dpr_raster_pullback_smooth_channels_ex", _lib.OP_PULLBACK, c, gt.shape[:n_out], algo,
            flags, workspace, gt, c["points"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg,
            d_ow, d_pw, tail=(C,))
    rot, trans, bg, ow = _per_pose(c, d_rot, d_trans, d_bg, d_ow)
    return PullbackResult(d_pts, rot, trans, bg, ow, d_pw)


class _RasterSmoothChannelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, point_weight, background, out_weight):
        out = raster_smooth_channels(grid_size, points.detach(), rotation.detach(), translation.detach(),
                                     _detach(point_weight), _detach(background), _detach(out_weight), algo=algo)
        _save(ctx, (points, rotation, translation), (point_weight, background, out_weight))
        # the pullback has DPR_ALGO_ATOMIC only: a forward on "tiled" differentiates on "auto"
        ctx.algo = "auto" if algo == "tiled" else algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation), opt = _restore(ctx, 3)
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, pw, bg, ow)
        pb = raster_pullback_smooth_channels_(ds_dout.detach(), points.detach(), rotation.detach(),
                                              translation.detach(), *map(_detach, opt), algo=ctx.algo,
                                              point_weight_grad=bool(ctx.opt_is_tensor[0] and need[5]))
        grads = (pb.points, pb.rotation, pb.translation, pb.point_weight, pb.background, pb.out_weight)
        return (None, None, *_cast_grads(need[2:], grads, (points, rotation, translation, *opt)))


def raster_smooth_channels_ad(grid_size, points, rotation, translation, point_weight, background=None,
                              out_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_smooth_channels` (torch autograd) in points, rotation, translation, point_weight,
    background and out_weight (whichever are tensors that require grad); the tangents are those of
    `raster_pullback_smooth_channels_`.  Reverse mode only."""
    return _RasterSmoothChannelsFn.apply(tuple(grid_size), algo, points, rotation, translation, point_weight,
                                         background, out_weight)
