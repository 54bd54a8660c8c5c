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

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from .interface import (_REFUSED, ColumnMajorRotation, DimensionMismatch, PullbackResult, _SUFFIX, _algo_name,
                        _allocate, _as, _canonicalise, _device_of, _grid_arr, _is_grid_layout, _promote, _ptr,
                        _stream_ptr, empty_grid, to_grid_layout)

MAX_CHANNELS = 16


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
    g = _grid_arr(grid_size)
    opc = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}[op]
    rc = _lib.lib().dpr_resolve_algo_channels(opc, n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p),
                                             n_points, batch, channels)
    return _algo_name(rc)


def workspace_bytes_channels(op: str, grid_size, n_points: int, batch: int, n_in: int, channels: int,
                             dtype=torch.float32, algo: str = "auto") -> int:
    """dpr_workspace_bytes_channels_ex_*: device bytes a channel call needs."""
    g = _grid_arr(grid_size)
    opc = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}[op]
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_channels_ex_{_SUFFIX[dtype]}")(
        opc, _lib.ALGOS[algo], 0, n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p), n_points, batch,
        channels)
    if need == _REFUSED:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, _lib.last_error())
    return int(need)


def _workspace(op, algo_c, suf, n_in, grid, P, B, C, device, workspace, flags):
    g = _grid_arr(grid)
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_channels_ex_{suf}")(
        op, algo_c, flags, n_in, len(grid), g.ctypes.data_as(ctypes.c_void_p), P, B, C)
    # (a refused query: the entry point itself reports the status, before any launch)
    return _allocate(0 if need == _REFUSED else need, device, workspace)


def _canonicalise_channels(points, rotation, translation, background, out_weight, point_weight, extra=()):
    """_canonicalise of interface.py plus the channel arguments: point_weight (P, C) -> C x P,
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
    device = _device_of(points)
    rot_like = isinstance(rotation, (torch.Tensor, ColumnMajorRotation))
    rot_nd = rotation.ndim if rot_like else torch.as_tensor(rotation).ndim
    dtype = _promote(points, rotation.cm if isinstance(rotation, ColumnMajorRotation) else rotation,
                     translation, background, out_weight, point_weight)
    batch = None if rot_nd == 2 else (rotation.shape[0] if rot_like else len(rotation))
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
    if not isinstance(out, torch.Tensor) or out.device != c["device"]:
        raise RuntimeError("out must be a tensor on the same HIP device as points")
    n_out, C, B = c["n_out"], c["C"], c["B"]
    expect_ndim = n_out + 1 + (0 if c["single"] else 1)
    if out.ndim != expect_ndim:
        raise DimensionMismatch(
            f"out has {out.ndim} dims, expected {expect_ndim} for N_out={n_out} and a channel axis")
    if out.shape[n_out] != C:
        raise DimensionMismatch(f"out channel dim {out.shape[n_out]} != number of channels {C}")
    if not c["single"] and out.shape[-1] != B:
        raise DimensionMismatch(f"out batch dim {out.shape[-1]} != number of poses {B}")
    if out.dtype != c["dtype"]:
        raise TypeError(f"out dtype {out.dtype} != promoted argument dtype {c['dtype']}")
    if not _is_grid_layout(out):
        raise ValueError("out must have the reference memory order (use empty_channel_grid)")
    grid = tuple(out.shape[:n_out])
    g = _grid_arr(grid)
    suf = _SUFFIX[c["dtype"]]
    algo_c = _lib.ALGOS[algo]
    with torch.cuda.device(c["device"]):
        ws, ws_bytes = _workspace(_lib.OP_RASTER, algo_c, suf, c["n_in"], grid, c["P"], B, C, c["device"],
                                  workspace, 0)
        fn = getattr(_lib.lib(), f"dpr_raster_channels_ex_{suf}")
        _lib.check(fn(_stream_ptr(c["device"]), algo_c, 0, c["n_in"], n_out, g.ctypes.data_as(ctypes.c_void_p),
                      c["P"], B, C, _ptr(out), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]),
                      _ptr(c["bg"]), _ptr(c["ow"]), _ptr(c["pw"]), _ptr(ws), ws_bytes))
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
    dev, dtype, P, B, C = c["device"], c["dtype"], c["P"], c["B"], c["C"]
    n_in, n_out = c["n_in"], c["n_out"]
    if not isinstance(ds_dout, torch.Tensor) or ds_dout.device != dev:
        raise RuntimeError("ds_dout must be a tensor on the same HIP device as points")
    expect_ndim = n_out + 1 + (0 if c["single"] else 1)
    if ds_dout.ndim != expect_ndim:
        raise DimensionMismatch(f"ds_dout has {ds_dout.ndim} dims, expected {expect_ndim}")
    if ds_dout.shape[n_out] != C:
        raise DimensionMismatch(f"ds_dout channel dim {ds_dout.shape[n_out]} != number of channels {C}")
    if not c["single"] and ds_dout.shape[-1] != B:
        raise DimensionMismatch(f"ds_dout batch dim {ds_dout.shape[-1]} != number of poses {B}")
    gt = ds_dout.to(dtype)
    if not _is_grid_layout(gt):
        gt = to_grid_layout(gt)
    grid = tuple(gt.shape[:n_out])
    g = _grid_arr(grid)

    def out_buf(given, shape, name):
        if given is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if (not isinstance(given, torch.Tensor) or given.device != dev or given.dtype != dtype
                or tuple(given.shape) != tuple(shape) or not given.is_contiguous()):
            raise DimensionMismatch(f"{name}: need a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
        return given

    d_pts = out_buf(ds_dpoints, (P, n_in), "ds_dpoints")
    if ds_drotation is not None:
        rv = ds_drotation.transpose(-1, -2) if not c["single"] else ds_drotation.t()[None]
        if rv.shape != (B, n_in, n_out) or not rv.is_contiguous() or rv.dtype != dtype:
            raise DimensionMismatch(
                "ds_drotation must be a (B, N_out, N_in) transposed view of a contiguous (B, N_in, N_out) buffer")
        d_rot = rv
    else:
        d_rot = torch.empty((B, n_in, n_out), dtype=dtype, device=dev)
    d_trans = out_buf(None if ds_dtranslation is None else ds_dtranslation.reshape(B, n_out), (B, n_out),
                      "ds_dtranslation")
    d_bg = out_buf(None if ds_dbackground is None else ds_dbackground.reshape(B, C), (B, C), "ds_dbackground")
    d_ow = out_buf(None if ds_dout_weight is None else ds_dout_weight.reshape(B), (B,), "ds_dout_weight")
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = out_buf(ds_dpoint_weight, (P, C), "ds_dpoint_weight") if point_weight_grad else None
    suf = _SUFFIX[dtype]
    algo_c = _lib.ALGOS[algo]
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    with torch.cuda.device(dev):
        ws, ws_bytes = _workspace(_lib.OP_PULLBACK, algo_c, suf, n_in, grid, P, B, C, dev, workspace, flags)
        fn = getattr(_lib.lib(), f"dpr_raster_pullback_channels_ex_{suf}")
        _lib.check(fn(_stream_ptr(dev), algo_c, flags, n_in, n_out, g.ctypes.data_as(ctypes.c_void_p), P, B, C,
                      _ptr(gt), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]), _ptr(c["ow"]),
                      _ptr(c["pw"]), _ptr(d_pts), _ptr(d_rot), _ptr(d_trans), _ptr(d_bg), _ptr(d_ow),
                      _ptr(d_pw), _ptr(ws), ws_bytes))
    rot_math = d_rot.transpose(1, 2)
    if c["single"]:
        return PullbackResult(d_pts, rot_math[0], d_trans[0], d_bg[0], d_ow[0], d_pw)
    return PullbackResult(d_pts, rot_math, d_trans, d_bg, d_ow, d_pw)


class _RasterChannelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, point_weight, background, out_weight):
        out = raster_channels(grid_size, points.detach(), rotation.detach(), translation.detach(),
                              point_weight.detach() if isinstance(point_weight, torch.Tensor) else point_weight,
                              background.detach() if isinstance(background, torch.Tensor) else background,
                              out_weight.detach() if isinstance(out_weight, torch.Tensor) else out_weight,
                              algo=algo)
        ctx.opt_is_tensor = tuple(isinstance(t, torch.Tensor) for t in (point_weight, background, out_weight))
        ctx.opt = tuple(None if isinstance(t, torch.Tensor) else t for t in (point_weight, background, out_weight))
        ctx.save_for_backward(points, rotation, translation,
                              *[t for t in (point_weight, background, out_weight) if isinstance(t, torch.Tensor)])
        # forward and pullback pick their algorithms independently (no binning is shared)
        ctx.algo = "atomic" if algo == "tiled" else algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        saved = list(ctx.saved_tensors)
        points, rotation, translation = saved[:3]
        rest = saved[3:]
        opt = [rest.pop(0) if ctx.opt_is_tensor[k] else ctx.opt[k] for k in range(3)]
        pw, bg, ow = opt
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, pw, bg, ow)
        pb = raster_pullback_channels_(ds_dout.detach(), points.detach(), rotation.detach(), translation.detach(),
                                       pw.detach() if isinstance(pw, torch.Tensor) else pw,
                                       bg.detach() if isinstance(bg, torch.Tensor) else bg,
                                       ow.detach() if isinstance(ow, torch.Tensor) else ow,
                                       algo=ctx.algo, point_weight_grad=bool(ctx.opt_is_tensor[0] and need[5]))
        grads = [None, None,
                 pb.points.to(points.dtype) if need[2] else None,
                 pb.rotation.to(rotation.dtype) if need[3] else None,
                 pb.translation.to(translation.dtype) if need[4] else None]
        for k, gr in enumerate((pb.point_weight, pb.background, pb.out_weight)):
            t = opt[k]
            if ctx.opt_is_tensor[k] and need[5 + k]:
                grads.append(gr.reshape(t.shape).to(t.dtype))
            else:
                grads.append(None)
        return tuple(grads)


def raster_channels_ad(grid_size, points, rotation, translation, point_weight, background=None, out_weight=None,
                       *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_channels` (torch autograd), like `raster_ad` without binning reuse.  Tensor
    arguments may require grad; the tangents are those of `raster_pullback_channels_`."""
    return _RasterChannelsFn.apply(tuple(grid_size), algo, points, rotation, translation, point_weight,
                                   background, out_weight)
