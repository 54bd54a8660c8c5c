"""Per-pose point clouds: a different cloud for every pose, forward and pullback
(dpr_raster_clouds_ex_* / dpr_raster_pullback_clouds_ex_*, include/dpr.h "PER-POSE CLOUDS").

For pose b, with its own cloud points[b]:

    out[i.., b] = background[b] + out_weight[b] * sum_p point_weight[b, p] * voxel_weight(i..; R_b points[b, p] + t_b)

Plane b is exactly `raster(grid, points[b], R_b, t_b, background[b], out_weight[b], point_weight[b])`, and the
pullback decomposes the same way (ds_dpoints[b] is the single-pose gradient of pose b: no sum over poses).  Shapes:

  points, ds_dpoints       (B, P, N_in) contiguous
  point_weight             (B, P), or (P,) shared by all poses; its gradient has the argument's shape ((P,): the
                           sum over the poses; (B, P) when point_weight is None)
  rotation, translation,   batched as in `raster`: (B, N_out, N_in), (B, N_out), (B,), (B,)
  background, out_weight
  out, ds_dout             grid_size + (B,) in the memory order of `empty_grid`

Clouds of different sizes: pad them to a common P with point_weight 0 (a zero-weight point deposits nothing and
gets ds_dpoints 0).
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (ColumnMajorRotation, DimensionMismatch, _alloc_like, _as, _canonicalise, _cast_grads, _detach,
                    _device_of, _image, _launch, _op_code, _out_buf, _resolve, _restore, _rotation_buf,
                    _save, _workspace_bytes, empty_grid)
from .interface import PullbackResult

_ACCEPTED_OPS = ("raster", "pullback")


def resolve_algo_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32) -> str:
    """Name of the algorithm `algo="auto"` picks for a per-pose cloud call (dpr_resolve_algo_clouds); op is
    "raster" or "pullback"; n_points is P, the points of each cloud.  The C query answers for fp32 data; an fp64
    pullback takes "atomic" where it answers "chunked" (include/dpr.h, PER-POSE CLOUDS)."""
    name = _resolve("dpr_resolve_algo_clouds", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch, n_in)
    return "atomic" if (op == "pullback" and dtype == torch.float64 and name == "chunked") else name


def workspace_bytes_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                           algo: str = "auto") -> int:
    """dpr_workspace_bytes_clouds_ex_*: device bytes a per-pose cloud call needs."""
    return _workspace_bytes("_clouds", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in)


def _shape(t):
    return tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(torch.as_tensor(t).shape)


def _check_shapes(points, rotation, translation, point_weight):
    """The shape errors of a per-pose cloud call, raised before anything else looks at the arguments."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor on a HIP device")
    if points.ndim != 3:
        raise DimensionMismatch(f"points must be (B, P, N_in), got {tuple(points.shape)}")
    B, P, n_in = points.shape
    rs = tuple(rotation.shape) if isinstance(rotation, (torch.Tensor, ColumnMajorRotation)) else _shape(rotation)
    if len(rs) != 3:
        raise DimensionMismatch(f"per-pose clouds need batched poses: rotation (B, N_out, N_in), got {rs}")
    if rs[0] != B:
        raise DimensionMismatch(f"points hold {B} clouds, but rotation has {rs[0]} poses")
    if rs[2] != n_in:
        raise DimensionMismatch(f"Column dimension of rotation (got {rs[2]}) and points (got {n_in}) must agree!")
    ts = _shape(translation)
    if ts != (B, rs[1]):
        raise DimensionMismatch(f"translation must be (B, N_out) = {(B, rs[1])}, got {ts}")
    if point_weight is not None and _shape(point_weight) not in ((B, P), (P,)):
        raise DimensionMismatch(
            f"size(point_weight) = {_shape(point_weight)} must be (B, P) = {(B, P)} or (P,) = {(P,)}")


def _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight, extra=()):
    """_canonicalise for (B, P, N_in) clouds: the pose arguments must be batched; point_weight
    (B, P) or (P,) becomes a contiguous (B, P) buffer.  Adds "shared_pw" (the argument was (P,))."""
    _check_shapes(points, rotation, translation, point_weight)
    device = _device_of(points)
    Bp, P, n_in = points.shape
    first = points[0] if Bp > 0 else points.new_empty((P, n_in))
    c = _canonicalise(first, rotation, translation, background, out_weight, None,
                      extra=(points, point_weight) + tuple(extra))
    B, dtype = c["B"], c["dtype"]
    if Bp != B:
        raise DimensionMismatch(f"points hold {Bp} clouds, but there are {B} poses")
    c["points"] = _as(points, dtype, device)
    c["shared_pw"] = False
    if point_weight is not None:
        shape = _shape(point_weight)
        if shape == (P,):
            c["shared_pw"] = True
            pw = _as(point_weight, dtype, device, (P,), "point_weight")
            c["pw"] = pw.unsqueeze(0).expand(B, P).contiguous()
        elif shape == (B, P):
            c["pw"] = _as(point_weight, dtype, device, (B, P), "point_weight")
        else:
            raise DimensionMismatch(f"size(point_weight) = {shape} must be (B, P) = {(B, P)} or (P,) = {(P,)}")
    return c


def raster_clouds(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                  *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N, b] (the layout of `empty_grid(grid_size, B)`)."""
    _check_shapes(points, rotation, translation, point_weight)
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), batch, dtype, device)
    return raster_clouds_(out, points, rotation, translation, background, out_weight, point_weight, algo=algo,
                          workspace=workspace)


def raster_clouds_(out, points, rotation, translation, background=None, out_weight=None, point_weight=None, *,
                   algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place forward: `out` (grid_size + (B,), memory order of `empty_grid`) is fully overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    _launch("_clouds", "dpr_raster_clouds_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, 0, workspace,
            out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    return out


def raster_pullback_clouds_(ds_dout, points, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                            ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None, algo: str = "auto",
                            workspace=None, point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_clouds`.  Keyword outputs are pre-allocated buffers, OVERWRITTEN and returned by
    identity: ds_dpoints (B, P, N_in); ds_drotation (B, N_out, N_in) as a transposed view of a contiguous
    (B, N_in, N_out) buffer; ds_dtranslation (B, N_out); ds_dbackground, ds_dout_weight (B,); ds_dpoint_weight
    shaped like point_weight ((P,): the sum over the poses; (B, P) when point_weight is None).
    `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither computed nor written
    and comes back as None."""
    c = _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight, extra=(ds_dout,))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    gr = _image(ds_dout, "ds_dout", c)
    d_pts = _out_buf(ds_dpoints, (B, P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c)
    d_bg = _out_buf(ds_dbackground, (B,), "ds_dbackground", c)
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c)
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = d_pw_user = None
    if point_weight_grad:
        if c["shared_pw"]:
            d_pw_user = _out_buf(ds_dpoint_weight, (P,), "ds_dpoint_weight", c)
            d_pw = torch.empty((B, P), dtype=c["dtype"], device=c["device"])
        else:
            d_pw = d_pw_user = _out_buf(ds_dpoint_weight, (B, P), "ds_dpoint_weight", c)
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    _launch("_clouds", "dpr_raster_pullback_clouds_ex", _lib.OP_PULLBACK, c, gr.shape[:n_out], algo, flags,
            workspace, gr, c["points"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg, d_ow,
            d_pw)
    if c["shared_pw"] and d_pw is not None:
        torch.sum(d_pw, dim=0, out=d_pw_user)  # a weight shared by all poses: the sum of its per-pose gradients
    return PullbackResult(d_pts, d_rot.transpose(1, 2), d_trans, d_bg, d_ow, d_pw_user)


class _RasterCloudsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, background, out_weight, point_weight):
        out = raster_clouds(grid_size, _detach(points), _detach(rotation), _detach(translation), _detach(background),
                            _detach(out_weight), _detach(point_weight), algo=algo)
        _save(ctx, (points, rotation, translation), (background, out_weight, point_weight))
        ctx.algo = algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation), opt = _restore(ctx, 3)
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_clouds_(ds_dout.detach(), _detach(points), _detach(rotation), _detach(translation),
                                     *map(_detach, opt), algo=ctx.algo,
                                     point_weight_grad=bool(ctx.opt_is_tensor[2] and need[7]))
        return (None, None, *_cast_grads(need[2:], pb, (points, rotation, translation, *opt)))


def raster_clouds_ad(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                     *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_clouds` (torch autograd) in points, rotation, translation, background, out_weight and
    point_weight (whichever are tensors that require grad); the tangents are those of `raster_pullback_clouds_`."""
    return _RasterCloudsFn.apply(tuple(grid_size), algo, points, rotation, translation, background, out_weight,
                                 point_weight)
