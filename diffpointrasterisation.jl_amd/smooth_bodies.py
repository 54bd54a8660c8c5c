"""The smooth splat of rigid bodies: `raster_bodies` with the quadratic B-spline weights of `raster_smooth`, forward
and pullback (dpr_raster_smooth_bodies_ex_* / dpr_raster_pullback_smooth_bodies_ex_*, include/dpr.h "SMOOTH SPLAT,
RIGID BODIES").

    out[i.., b] = background[b]
                + out_weight[b] * sum_p point_weight[p] * Bspline_weight(i..; R[b, body[p]] points[p] + t[b, body[p]])

With background 0, plane b is the sum over k of `raster_smooth` of the points with body == k under pose (b, k); every
gradient is the matching piece of `raster_pullback_smooth_` of that subset, and the pullback is the exact derivative:
the operator is C1 in the points and in all B * K poses.  One call in the place of K subset calls, or of B warped
copies of the cloud through `raster_smooth_clouds`.

Shapes are those of `raster_bodies`: points (P, N_in); body (P,) int32 or int64, no gradient; rotation
(B, K, N_out, N_in) and translation (B, K, N_out), or without the B axis for one image; background, out_weight (B,),
a scalar for one image, or None; point_weight (P,) or None.  A point whose body lies outside [0, K) is dropped: it
deposits nothing and gets zero gradients.  Sort the cloud by body.  (N_in, N_out): (2,2), (3,3), (3,2).

Algorithms: "atomic" (forward and pullback), "tiled" (forward: the images are binned in groups, four launches per
group; `max_pose_group` bounds a group), "auto".  There is no public workspace query for this family: every call
asks dpr_workspace_bytes_smooth_bodies_ex_* itself and allocates, or checks the `workspace` the caller passed (a uint8
tensor on the device); the C query is reachable through `lib()`.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (_cast_grads, _detach, _device_of, _image, _launch, _op_code, _out_buf, _promote, _resolve,
                    _restore, _save, empty_grid)
from .bodies import _canonicalise_bodies, _check_shapes, _rotation_buf
from .interface import PullbackResult

_ACCEPTED_OPS = ("raster", "pullback")


def resolve_algo_smooth_bodies(op: str, grid_size, n_points: int, batch: int, n_bodies: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth rigid-body call (dpr_resolve_algo_smooth_bodies); op is
    "raster" or "pullback"."""
    return _resolve("dpr_resolve_algo_smooth_bodies", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch,
                    n_in, n_bodies)


def raster_smooth_bodies(grid_size, points, body, rotation, translation, background=None, out_weight=None,
                         point_weight=None, *, algo: str = "auto", workspace=None,
                         max_pose_group: int = 0) -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N(, b)] (the layout of `empty_grid`)."""
    single, B, _K, _n_out, _n_in = _check_shapes(points, body, rotation, translation, point_weight)
    _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything is allocated)
    device = _device_of(points)
    dtype = _promote(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), None if single else B, dtype, device)
    return raster_smooth_bodies_(out, points, body, rotation, translation, background, out_weight, point_weight,
                                 algo=algo, workspace=workspace, max_pose_group=max_pose_group)


def raster_smooth_bodies_(out, points, body, rotation, translation, background=None, out_weight=None,
                          point_weight=None, *, algo: str = "auto", workspace=None,
                          max_pose_group: int = 0) -> torch.Tensor:
    """In-place forward: `out` (grid_size (+ (B,)), memory order of `empty_grid`) is fully overwritten and returned.
    `max_pose_group` (1..16, 0 = default): the most images "tiled" bins together (DPR_FLAG_MAX_POSE_GROUP).  Enqueued
    on torch's current stream; not synchronised."""
    _check_shapes(points, body, rotation, translation, point_weight)
    flags = _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything else)
    c = _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    _launch("_smooth_bodies", "dpr_raster_smooth_bodies_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, flags,
            workspace, out, c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], tail=(c["K"],))
    return out


def raster_pullback_smooth_bodies_(ds_dout, points, body, rotation, translation, background=None, out_weight=None,
                                   point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                                   ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None,
                                   algo: str = "auto", point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_smooth_bodies`.  Keyword outputs are pre-allocated buffers, OVERWRITTEN and returned by
    identity, with the shapes of `raster_pullback_bodies_`: ds_dpoints (P, N_in); ds_drotation shaped like rotation,
    a transposed view of a contiguous (B, K, N_in, N_out) buffer; ds_dtranslation (B, K, N_out); ds_dbackground,
    ds_dout_weight (B,); ds_dpoint_weight (P,).  For one image (rotation (K, N_out, N_in)) the B axis is absent
    everywhere.  `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither computed
    nor written and comes back as None."""
    c = _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight,
                             extra=(ds_dout,))
    P, B, K, n_in, n_out, single = c["P"], c["B"], c["K"], c["n_in"], c["n_out"], c["single"]
    gr = _image(ds_dout, "ds_dout", c)
    d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    d_trans = _out_buf(ds_dtranslation, (B, K, n_out), "ds_dtranslation", c, reshape=single)
    d_bg = _out_buf(ds_dbackground, (B,), "ds_dbackground", c, reshape=single)
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c, reshape=single)
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = _out_buf(ds_dpoint_weight, (P,), "ds_dpoint_weight", c) if point_weight_grad else None
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    _launch("_smooth_bodies", "dpr_raster_pullback_smooth_bodies_ex", _lib.OP_PULLBACK, c, gr.shape[:n_out], algo,
            flags, None, gr, c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans,
            d_bg, d_ow, d_pw, tail=(K,))
    rot = d_rot.transpose(-1, -2)
    if single:
        rot, d_trans, d_bg, d_ow = rot[0], d_trans[0], d_bg[0], d_ow[0]
    return PullbackResult(d_pts, rot, d_trans, d_bg, d_ow, d_pw)


class _SmoothBodiesJvpFn(torch.autograd.Function):
    """`raster_smooth_bodies_jvp` as one opaque call with plain device tensors, for `_RasterSmoothBodiesFn.jvp`: under
    torch.func transforms the tangents arrive wrapped, and a function is what unwraps them.  Not differentiable."""

    @staticmethod
    def forward(grid_size, algo, body, points, rotation, translation, background, out_weight, point_weight,
                points_t, rotation_t, translation_t, background_t, out_weight_t, point_weight_t):
        from .smooth_bodies_jvp import raster_smooth_bodies_jvp  # (smooth_bodies_jvp imports the bodies family)

        return raster_smooth_bodies_jvp(grid_size, points, body, rotation, translation, background, out_weight,
                                        point_weight, points_dot=points_t, rotation_dot=rotation_t,
                                        translation_dot=translation_t, background_dot=background_t,
                                        out_weight_dot=out_weight_t, point_weight_dot=point_weight_t, algo=algo)

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass


class _RasterSmoothBodiesFn(torch.autograd.Function):
    # (forward and setup_context apart: what torch.func.jvp asks of a function)
    @staticmethod
    def forward(grid_size, algo, body, points, rotation, translation, background, out_weight, point_weight):
        return raster_smooth_bodies(grid_size, _detach(points), body, _detach(rotation), _detach(translation),
                                    _detach(background), _detach(out_weight), _detach(point_weight), algo=algo)

    @staticmethod
    def setup_context(ctx, inputs, output):
        grid_size, algo, body, points, rotation, translation, background, out_weight, point_weight = inputs
        saved = _save(ctx, (points, rotation, translation, body), (background, out_weight, point_weight))
        ctx.save_for_forward(*saved)
        ctx.grid_size, ctx.caller_algo = tuple(int(n) for n in grid_size), algo
        # the pullback has DPR_ALGO_ATOMIC only: a forward on "tiled" differentiates on "auto"
        ctx.algo = "auto" if algo == "tiled" else algo

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation, body), opt = _restore(ctx, 4)
        need = ctx.needs_input_grad  # (grid_size, algo, body, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_smooth_bodies_(ds_dout.detach(), _detach(points), body, _detach(rotation),
                                            _detach(translation), *map(_detach, opt), algo=ctx.algo,
                                            point_weight_grad=bool(ctx.opt_is_tensor[2] and need[8]))
        return (None, None, None, *_cast_grads(need[3:], pb, (points, rotation, translation, *opt)))

    @staticmethod
    def jvp(ctx, _grid_t, _algo_t, _body_t, points_t, rotation_t, translation_t, background_t, out_weight_t,
            point_weight_t):
        (points, rotation, translation, body), opt = _restore(ctx, 4)
        algo = ctx.caller_algo if ctx.caller_algo in ("atomic", "tiled") else "auto"
        return _SmoothBodiesJvpFn.apply(ctx.grid_size, algo, body, _detach(points), _detach(rotation),
                                        _detach(translation), *map(_detach, opt), points_t, rotation_t, translation_t,
                                        background_t, out_weight_t, point_weight_t)


def raster_smooth_bodies_ad(grid_size, points, body, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_smooth_bodies` (torch autograd) in points, rotation, translation, background,
    out_weight and point_weight (whichever are tensors that require grad); `body` has no gradient.  The tangents are
    those of `raster_pullback_smooth_bodies_`.  Forward mode (torch.autograd.forward_ad dual tensors, torch.func.jvp)
    goes through `raster_smooth_bodies_jvp` with one tangent, on the caller's algorithm ("atomic" / "tiled") or
    AUTO."""
    return _RasterSmoothBodiesFn.apply(tuple(grid_size), algo, body, points, rotation, translation, background,
                                       out_weight, point_weight)
