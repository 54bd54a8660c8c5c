"""Rigid bodies: one cloud whose points belong to K bodies, each with its own pose in every image, forward and
pullback (dpr_raster_bodies_ex_* / dpr_raster_pullback_bodies_ex_*, include/dpr.h "RIGID BODIES").

    out[i.., b] = background[b]
                + out_weight[b] * sum_p point_weight[p] * voxel_weight(i..; R[b, body[p]] points[p] + t[b, body[p]])

With background 0, plane b is the sum over k of `raster` of the points with body == k under pose (b, k); every
gradient is the matching piece of `raster_pullback_` of that subset (ds_dout_weight adds over k).  Shapes:

  points, ds_dpoints           (P, N_in)
  body                         (P,) int32 or int64 on the device (int64 is narrowed to an int32 copy, indices
                               beyond int32 staying out of range); no gradient
  rotation, ds_drotation       (B, K, N_out, N_in), or (K, N_out, N_in) for one image
  translation, ds_dtranslation (B, K, N_out), or (K, N_out)
  background, out_weight       (B,), a scalar for one image, or None; their gradients alike
  point_weight                 (P,) or None
  out, ds_dout                 grid_size (+ (B,)) in the memory order of `empty_grid`

A point whose body lies outside [0, K) is dropped: it deposits nothing and gets zero gradients.  Sort the cloud by
body: a wave of 64 consecutive points that share one body reads its pose once and reduces its pose gradients
together.  (N_in, N_out) is (2, 2), (3, 3) or (3, 2).
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (DimensionMismatch, _as, _canonicalise, _cast_grads, _detach, _device_of, _image, _launch,
                    _op_code, _out_buf, _promote, _resolve, _restore, _save, _scalar, empty_grid)
from .interface import PullbackResult

_ACCEPTED_OPS = ("raster", "pullback")
_PAIRS = ((2, 2), (3, 3), (3, 2))


def resolve_algo_bodies(op: str, grid_size, n_points: int, batch: int, n_bodies: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a rigid-body call (dpr_resolve_algo_bodies): "atomic" for
    every call the library accepts; op is "raster" or "pullback"."""
    return _resolve("dpr_resolve_algo_bodies", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch, n_in,
                    n_bodies)


def _shape(t):
    return tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(torch.as_tensor(t).shape)


def _check_shapes(points, body, rotation, translation, point_weight=None):
    """The shape errors of a rigid-body call, raised before anything else looks at the arguments.  Returns
    (single, B, K, N_out, N_in)."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor on a HIP device")
    if points.ndim != 2:
        raise DimensionMismatch(f"points must be (P, N_in), got {tuple(points.shape)}")
    P, n_in = points.shape
    if not isinstance(body, torch.Tensor) or body.dtype not in (torch.int32, torch.int64):
        raise TypeError("body must be an int32 or int64 torch.Tensor")
    if tuple(body.shape) != (P,):
        raise DimensionMismatch(f"body must be (P,) = {(P,)}, got {tuple(body.shape)}")
    rs, ts = _shape(rotation), _shape(translation)
    if len(rs) not in (3, 4):
        raise DimensionMismatch(f"rotation must be (B, K, N_out, N_in) or (K, N_out, N_in), got {rs}")
    single = len(rs) == 3
    B, (K, n_out, n_in_rot) = (1 if single else rs[0]), rs[-3:]
    if K < 1:
        raise DimensionMismatch(f"rotation holds K = {K} bodies: a call needs at least one")
    if n_in_rot != n_in:
        raise DimensionMismatch(f"Column dimension of rotation (got {n_in_rot}) and points (got {n_in}) must agree!")
    if ts != rs[:-1]:
        raise DimensionMismatch(f"translation must be {rs[:-1]} (rotation without its last axis), got {ts}")
    if (n_in, n_out) not in _PAIRS:
        raise DimensionMismatch(f"rigid bodies support (N_in, N_out) in {_PAIRS}, got {(n_in, n_out)}")
    if point_weight is not None and _shape(point_weight) != (P,):
        raise DimensionMismatch(f"length(point_weight) = {_shape(point_weight)} != n_points = {P}")
    return single, B, K, n_out, n_in


def _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight, extra=()):
    """_canonicalise with a K axis in the poses: "rot" / "trans" hold the B * K poses, pose (b, k) at b * K + k;
    adds "K" and "body" (contiguous int32 on the device)."""
    single, B, K, n_out, n_in = _check_shapes(points, body, rotation, translation, point_weight)
    device = _device_of(points)
    rot = rotation if isinstance(rotation, torch.Tensor) else torch.as_tensor(rotation)
    trans = translation if isinstance(translation, torch.Tensor) else torch.as_tensor(translation)
    # the B * K poses as one batch; background and out_weight (per image) take part in the promotion only
    c = _canonicalise(points, rot.reshape(B * K, n_out, n_in), trans.reshape(B * K, n_out), None, None,
                      point_weight, extra=(background, out_weight) + tuple(extra))
    if single:
        background = None if background is None else _scalar(background)
        out_weight = None if out_weight is None else _scalar(out_weight)
    dtype = c["dtype"]
    c["bg"] = None if background is None else _as(background, dtype, device, (B,), "background")
    c["ow"] = None if out_weight is None else _as(out_weight, dtype, device, (B,), "out_weight")
    if body.device != device:
        raise RuntimeError("body must be a tensor on the same HIP device as points")
    # (int64: indices beyond int32 must stay outside [0, K) when they are narrowed; K < 2^31)
    c["body"] = (body if body.dtype == torch.int32 else body.clamp(-1, K).to(torch.int32)).contiguous()
    c.update(single=single, B=B, K=K)
    return c


def _rotation_buf(given, c):
    """The ds_drotation output: the caller's (B, K, N_out, N_in) ((K, N_out, N_in) for one image) transposed view
    of a contiguous (B, K, N_in, N_out) buffer -- column-major N_out x N_in per pose, as the C ABI has it -- or a
    new one."""
    B, K, n_in, n_out = c["B"], c["K"], c["n_in"], c["n_out"]
    if given is None:
        return torch.empty((B, K, n_in, n_out), dtype=c["dtype"], device=c["device"])
    rv = given.transpose(-1, -2)
    rv = rv[None] if c["single"] else rv
    if (tuple(rv.shape) != (B, K, n_in, n_out) or not rv.is_contiguous() or rv.dtype != c["dtype"]
            or rv.device != c["device"]):
        raise DimensionMismatch(
            f"ds_drotation must be a (B, K, N_out, N_in) transposed view of a contiguous (B, K, N_in, N_out) "
            f"{c['dtype']} buffer on {c['device']} (column-major N_out x N_in per pose)")
    return rv


def raster_bodies(grid_size, points, body, rotation, translation, background=None, out_weight=None,
                  point_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N(, b)] (the layout of `empty_grid`)."""
    single, B, _K, _n_out, _n_in = _check_shapes(points, body, rotation, translation, point_weight)
    device = _device_of(points)
    dtype = _promote(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), None if single else B, dtype, device)
    return raster_bodies_(out, points, body, rotation, translation, background, out_weight, point_weight, algo=algo)


def raster_bodies_(out, points, body, rotation, translation, background=None, out_weight=None, point_weight=None,
                   *, algo: str = "auto") -> torch.Tensor:
    """In-place forward: `out` (grid_size (+ (B,)), memory order of `empty_grid`) is fully overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    _launch("_bodies", "dpr_raster_bodies_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, 0, None,
            out, c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], tail=(c["K"],))
    return out


def raster_pullback_bodies_(ds_dout, points, body, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                            ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None, algo: str = "auto",
                            point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_bodies`.  Keyword outputs are pre-allocated buffers, OVERWRITTEN and returned by
    identity: ds_dpoints (P, N_in); ds_drotation shaped like rotation, a transposed view of a contiguous
    (B, K, N_in, N_out) buffer; ds_dtranslation (B, K, N_out); ds_dbackground, ds_dout_weight (B,);
    ds_dpoint_weight (P,).  For one image (rotation (K, N_out, N_in)) the B axis is absent everywhere.
    `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither computed nor written
    and comes back as None."""
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
    _launch("_bodies", "dpr_raster_pullback_bodies_ex", _lib.OP_PULLBACK, c, gr.shape[:n_out], algo, flags, None,
            gr, c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"], d_pts, d_rot, d_trans, d_bg, d_ow,
            d_pw, tail=(K,))
    rot = d_rot.transpose(-1, -2)
    if single:
        rot, d_trans, d_bg, d_ow = rot[0], d_trans[0], d_bg[0], d_ow[0]
    return PullbackResult(d_pts, rot, d_trans, d_bg, d_ow, d_pw)


class _RasterBodiesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, body, points, rotation, translation, background, out_weight, point_weight):
        out = raster_bodies(grid_size, _detach(points), body, _detach(rotation), _detach(translation),
                            _detach(background), _detach(out_weight), _detach(point_weight), algo=algo)
        _save(ctx, (points, rotation, translation, body), (background, out_weight, point_weight))
        ctx.algo = algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        (points, rotation, translation, body), opt = _restore(ctx, 4)
        need = ctx.needs_input_grad  # (grid_size, algo, body, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_bodies_(ds_dout.detach(), _detach(points), body, _detach(rotation),
                                     _detach(translation), *map(_detach, opt), algo=ctx.algo,
                                     point_weight_grad=bool(ctx.opt_is_tensor[2] and need[8]))
        return (None, None, None, *_cast_grads(need[3:], pb, (points, rotation, translation, *opt)))


def raster_bodies_ad(grid_size, points, body, rotation, translation, background=None, out_weight=None,
                     point_weight=None, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_bodies` (torch autograd) in points, rotation, translation, background, out_weight and
    point_weight (whichever are tensors that require grad); `body` has no gradient.  The tangents are those of
    `raster_pullback_bodies_`."""
    return _RasterBodiesFn.apply(tuple(grid_size), algo, body, points, rotation, translation, background, out_weight,
                                 point_weight)
