"""The smooth splat of per-pose point clouds: `raster_smooth` with a different cloud for every pose, forward and
pullback (dpr_raster_smooth_clouds_ex_* / dpr_raster_pullback_smooth_clouds_ex_*, include/dpr.h "SMOOTH SPLAT,
PER-POSE CLOUDS").

For pose b, with its own cloud points[b]:

    out[i.., b] = background[b] + out_weight[b] * sum_p point_weight[b, p] * Bspline_weight(i..; R_b points[b, p] + t_b)

Plane b is exactly `raster_smooth(grid, points[b], R_b, t_b, background[b], out_weight[b], point_weight[b])`, and the
pullback -- the exact derivative, the operator is C1 -- decomposes the same way (ds_dpoints[b] is the single-pose
smooth gradient of pose b: no sum over poses).  One call in the place of a Python loop of B single-pose calls; on
"tiled" the poses are binned in groups, four launches per group instead of four per pose.

Shapes are those of `raster_clouds`: points (B, P, N_in); point_weight (B, P), or (P,) shared by all poses (its
gradient is then the sum over the poses); rotation, translation, background, out_weight batched.  (N_in, N_out):
(2,2), (3,3), (3,2).  Algorithms: "atomic" (forward and pullback), "tiled" (forward), "auto".  Clouds of different
sizes: pad them to a common P with point_weight 0 (a zero-weight point deposits nothing and gets ds_dpoints 0).
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (ColumnMajorRotation, DimensionMismatch, _alloc_like, _cast_grads, _detach, _image, _launch,
                    _op_code, _out_buf, _resolve, _restore, _rotation_buf, _save, _workspace_bytes, empty_grid)
from .clouds import _canonicalise_clouds
from .clouds import _check_shapes as _check_cloud_shapes
from .interface import PullbackResult
from .smooth import _PAIRS

_ACCEPTED_OPS = ("raster", "pullback")


def resolve_algo_smooth_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth per-pose cloud call (dpr_resolve_algo_smooth_clouds);
    op is "raster" or "pullback"; n_points is P, the points of each cloud."""
    return _resolve("dpr_resolve_algo_smooth_clouds", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch,
                    n_in)


def workspace_bytes_smooth_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                                  algo: str = "auto", max_pose_group: int = 0) -> int:
    """dpr_workspace_bytes_smooth_clouds_ex_*: device bytes a smooth per-pose cloud call needs.  `max_pose_group`
    (1..16, 0 = default) must be the value the call itself will carry."""
    return _workspace_bytes("_smooth_clouds", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo],
                                               _lib.flag_max_pose_group(max_pose_group)),
                            dtype, grid_size, n_points, batch, n_in)


def _check_shapes(points, rotation, translation, point_weight):
    """The shape and dimension errors of a call, raised before anything else looks at the arguments (and before any
    library call): those of per-pose clouds, then the (N_in, N_out) pairs the smooth splat has."""
    _check_cloud_shapes(points, rotation, translation, point_weight)
    rs = tuple(rotation.shape) if isinstance(rotation, (torch.Tensor, ColumnMajorRotation)) \
        else tuple(torch.as_tensor(rotation).shape)
    if (rs[2], rs[1]) not in _PAIRS:
        raise DimensionMismatch(f"raster_smooth_clouds supports (N_in, N_out) in {_PAIRS}, got {(rs[2], rs[1])}")


def _canonicalise_smooth_clouds(points, rotation, translation, background, out_weight, point_weight, extra=()):
    _check_shapes(points, rotation, translation, point_weight)
    return _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight, extra=extra)


def raster_smooth_clouds(grid_size, points, rotation, translation, background=None, out_weight=None,
                         point_weight=None, *, algo: str = "auto", workspace=None,
                         max_pose_group: int = 0) -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N, b] (the layout of `empty_grid(grid_size, B)`)."""
    _check_shapes(points, rotation, translation, point_weight)
    _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything is allocated)
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), batch, dtype, device)
    return raster_smooth_clouds_(out, points, rotation, translation, background, out_weight, point_weight,
                                 algo=algo, workspace=workspace, max_pose_group=max_pose_group)


def raster_smooth_clouds_(out, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                          *, algo: str = "auto", workspace=None, max_pose_group: int = 0) -> torch.Tensor:
    """In-place forward: `out` (grid_size + (B,), memory order of `empty_grid`) is fully overwritten and returned.
    `max_pose_group` (1..16, 0 = default): the most poses "tiled" bins together (DPR_FLAG_MAX_POSE_GROUP).  Enqueued
    on torch's current stream; not synchronised."""
    _check_shapes(points, rotation, translation, point_weight)
    flags = _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything else)
    c = _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    _launch("_smooth_clouds", "dpr_raster_smooth_clouds_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo,
            flags, workspace, out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    return out


def raster_pullback_smooth_clouds_(ds_dout, points, rotation, translation, background=None, out_weight=None,
                                   point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                                   ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None,
                                   algo: str = "auto", workspace=None,
                                   point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_smooth_clouds`.  Keyword outputs are pre-allocated buffers, OVERWRITTEN and returned by
    identity, with the shapes of `raster_pullback_clouds_`: ds_dpoints (B, P, N_in); ds_drotation (B, N_out, N_in) as
    a transposed view of a contiguous (B, N_in, N_out) buffer; ds_dtranslation (B, N_out); ds_dbackground,
    ds_dout_weight (B,); ds_dpoint_weight shaped like point_weight ((P,): the sum over the poses; (B, P) when
    point_weight is None).  `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither
    computed nor written and comes back as None."""
    c = _canonicalise_smooth_clouds(points, rotation, translation, background, out_weight, point_weight,
                                    extra=(ds_dout,))
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
    _launch("_smooth_clouds", "dpr_raster_pullback_smooth_clouds_ex", _lib.OP_PULLBACK, c, gr.shape[:n_out], algo,
            flags, workspace, gr, c["points"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg,
            d_ow, d_pw)
    if c["shared_pw"] and d_pw is not None:
        torch.sum(d_pw, dim=0, out=d_pw_user)  # a weight shared by all poses: the sum of its per-pose gradients
    return PullbackResult(d_pts, d_rot.transpose(1, 2), d_trans, d_bg, d_ow, d_pw_user)


class _RasterSmoothCloudsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, background, out_weight, point_weight):
        out = raster_smooth_clouds(grid_size, _detach(points), _detach(rotation), _detach(translation),
                                   _detach(background), _detach(out_weight), _detach(point_weight), algo=algo)
        _save(ctx, (points, rotation, translation), (background, out_weight, point_weight))
        # the pullback has DPR_ALGO_ATOMIC only: a forward on "tiled" differentiates on "auto"
        ctx.algo = "auto" if algo == "tiled" else algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation), opt = _restore(ctx, 3)
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_smooth_clouds_(ds_dout.detach(), _detach(points), _detach(rotation),
                                            _detach(translation), *map(_detach, opt), algo=ctx.algo,
                                            point_weight_grad=bool(ctx.opt_is_tensor[2] and need[7]))
        return (None, None, *_cast_grads(need[2:], pb, (points, rotation, translation, *opt)))


def raster_smooth_clouds_ad(grid_size, points, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_smooth_clouds` (torch autograd) in points, rotation, translation, background,
    out_weight and point_weight (whichever are tensors that require grad); the tangents are those of
    `raster_pullback_smooth_clouds_`."""
    return _RasterSmoothCloudsFn.apply(tuple(grid_size), algo, points, rotation, translation, background, out_weight,
                                       point_weight)
