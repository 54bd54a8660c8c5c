"""Multi-channel rasterisation: C weights per point into (grid..., C[, B]) images, forward and pullback
(dpr_raster_channels_ex_* / dpr_raster_pullback_channels_ex_*, include/dpr.h "MULTI-CHANNEL").

For channel c and pose b

    out[i.., c, b] = background[b, c] + out_weight[b] * sum_p point_weight[p, c] * voxel_weight(i..; R_b p + t_b)

i.e. plane c is `raster(..., background=background[..., c], point_weight=point_weight[:, c])`.  Shapes:

  point_weight  (P, C)                       memory C x P, channel fastest (Vector{SVector{C,T}})
  background    (C,) single pose, (B, C)     memory C x B
  out, ds_dout  grid_size + (C,) [+ (B,)]    memory of a contiguous (B, C, n_N, .., n_1) tensor (NCHW /
                                             NCDHW): `empty_channel_grid` allocates it

Everything else is as for `raster` / `raster_pullback_`; out_weight is one scalar per pose, shared by the
channels.  The pullback's ds_dpoints / rotation / translation / out_weight are sums over the channels,
point_weight (P, C) and background (C,) / (B, C) are per channel.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib
from ._args import (DimensionMismatch, _alloc_like, _as, _canonicalise, _cast_grads, _detach, _image, _launch,
                    _op_code, _out_buf, _per_pose, _resolve, _restore, _rotation_buf, _save, _workspace_bytes,
                    empty_grid)
from .interface import PullbackResult

MAX_CHANNELS = 16
_ACCEPTED_OPS = ("raster", "pullback")


def empty_channel_grid(grid_size: Sequence[int], channels: int, batch: Optional[int], dtype,
                       device) -> torch.Tensor:
    """Allocate an `out` / `ds_dout` of the channel entry points: a view of logical shape
    grid_size + (C,) (+ (B,)) whose memory is a contiguous (B, C, n_N, .., n_1) tensor."""
    return empty_grid(tuple(int(n) for n in grid_size) + (int(channels),), batch, dtype, device)


def _check_channels(C):
    if not 1 <= int(C) <= MAX_CHANNELS:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, f"channels C = {C} out of range [1, {MAX_CHANNELS}]")


def resolve_algo_channels(op: str, grid_size, n_points: int, batch: int, n_in: int, channels: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a channel call (dpr_resolve_algo_channels)."""
    return _resolve("dpr_resolve_algo_channels", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch, n_in,
                    channels)


def workspace_bytes_channels(op: str, grid_size, n_points: int, batch: int, n_in: int, channels: int,
                             dtype=torch.float32, algo: str = "auto") -> int:
    """dpr_workspace_bytes_channels_ex_*: device bytes a channel call needs."""
    return _workspace_bytes("_channels", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in, channels)


def _canonicalise_channels(points, rotation, translation, background, out_weight, point_weight, extra=()):
    """_canonicalise plus the channel arguments: point_weight (P, C) -> C x P,
    background (C,) / (B, C) -> C x B.  Returns the dict of _canonicalise with C, bg, pw set."""
    c = _canonicalise(points, rotation, translation, None, out_weight, None,
                      extra=(background, point_weight) + tuple(extra))
    P, B, dtype, dev = c["P"], c["B"], c["dtype"], c["device"]
    if point_weight is None:
        raise DimensionMismatch("point_weight: the channel API needs a (P, C) point_weight (C = its last dim)")
    pw_shape = tuple(torch.as_tensor(point_weight).shape) if not isinstance(point_weight, torch.Tensor) \
        else tuple(point_weight.shape)
    if len(pw_shape) != 2 or pw_shape[0] != P:
        raise DimensionMismatch(  # (the channel form of @argcheck length(point_weight) == n_points)
            f"size(point_weight) = {pw_shape} must be (n_points = {P}, C)")
    C = pw_shape[1]
    _check_channels(C)
    c["C"] = C
    c["pw"] = _as(point_weight, dtype, dev, (P, C), "point_weight")
    if background is None:
        c["bg"] = None
    else:
        bshape = tuple(background.shape) if isinstance(background, torch.Tensor) else \
            tuple(torch.as_tensor(background).shape)
        want = (C,) if c["single"] else (B, C)
        if bshape != want:
            raise DimensionMismatch(
                f"size(background) = {bshape} must be {want} ({'C' if c['single'] else 'B x C'} with C = {C})")
        c["bg"] = _as(background, dtype, dev, want, "background").reshape(B, C).contiguous()
    return c


def _infer_channels(point_weight):
    shape = tuple(point_weight.shape) if isinstance(point_weight, torch.Tensor) else \
        tuple(torch.as_tensor(point_weight).shape)
    if len(shape) != 2:
        raise DimensionMismatch(f"size(point_weight) = {shape} must be (n_points, C)")
    return shape[1]


def raster_channels(grid_size, points, rotation, translation, point_weight, background=None, out_weight=None,
                    *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating multi-channel forward: returns out[i_1..i_N, c] (single pose) or out[i_1..i_N, c, b]."""
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    C = _infer_channels(point_weight)
    _check_channels(C)
    out = empty_channel_grid(tuple(grid_size), C, batch, dtype, device)
    return raster_channels_(out, points, rotation, translation, point_weight, background, out_weight,
                            algo=algo, workspace=workspace)


def raster_channels_(out, points, rotation, translation, point_weight, background=None, out_weight=None,
                     *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place multi-channel forward: `out` (grid_size + (C,) [+ (B,)], `empty_channel_grid` memory order)
    is fully overwritten and returned.  Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_channels(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, (("channels", c["C"]),), out=True)
    _launch("_channels", "dpr_raster_channels_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, 0, workspace,
            out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], tail=(c["C"],))
    return out


def raster_pullback_channels_(ds_dout, points, rotation, translation, point_weight, background=None,
                              out_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                              ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None,
                              algo: str = "auto", workspace=None, point_weight_grad: bool = True) -> PullbackResult:
    """Multi-channel pullback.  Keyword outputs as for `raster_pullback_` (overwritten, returned by
    identity) except ds_dpoint_weight (P, C) and ds_dbackground (C,) / (B, C).  Returns PullbackResult with
    point_weight (P, C) (None with point_weight_grad=False) and background (C,) or (B, C)."""
    c = _canonicalise_channels(points, rotation, translation, background, out_weight, point_weight,
                               extra=(ds_dout,))
    P, B, C, n_in, n_out = c["P"], c["B"], c["C"], c["n_in"], c["n_out"]
    gt = _image(ds_dout, "ds_dout", c, (("channels", C),))
    d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=True)
    d_bg = _out_buf(ds_dbackground, (B, C), "ds_dbackground", c, reshape=True)
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c, reshape=True)
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = _out_buf(ds_dpoint_weight, (P, C), "ds_dpoint_weight", c) if point_weight_grad else None
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    _launch("_channels", "dpr_raster_pullback_channels_ex", _lib.OP_PULLBACK, c, gt.shape[:n_out], algo, flags,
            workspace, gt, c["points"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg, d_ow,
            d_pw, tail=(C,))
    rot, trans, bg, ow = _per_pose(c, d_rot, d_trans, d_bg, d_ow)
    return PullbackResult(d_pts, rot, trans, bg, ow, d_pw)


class _RasterChannelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, point_weight, background, out_weight):
        out = raster_channels(grid_size, points.detach(), rotation.detach(), translation.detach(),
                              _detach(point_weight), _detach(background), _detach(out_weight), algo=algo)
        _save(ctx, (points, rotation, translation), (point_weight, background, out_weight))
        # forward and pullback pick their algorithms independently (no binning is shared)
        ctx.algo = "atomic" if algo == "tiled" else algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation), opt = _restore(ctx, 3)
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, pw, bg, ow)
        pb = raster_pullback_channels_(ds_dout.detach(), points.detach(), rotation.detach(), translation.detach(),
                                       *map(_detach, opt), algo=ctx.algo,
                                       point_weight_grad=bool(ctx.opt_is_tensor[0] and need[5]))
        grads = (pb.points, pb.rotation, pb.translation, pb.point_weight, pb.background, pb.out_weight)
        return (None, None, *_cast_grads(need[2:], grads, (points, rotation, translation, *opt)))


def raster_channels_ad(grid_size, points, rotation, translation, point_weight, background=None, out_weight=None,
                       *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_channels` (torch autograd), like `raster_ad` without binning reuse.  Tensor
    arguments may require grad; the tangents are those of `raster_pullback_channels_`."""
    return _RasterChannelsFn.apply(tuple(grid_size), algo, points, rotation, translation, point_weight,
                                   background, out_weight)
