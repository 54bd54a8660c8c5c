"""Forward-mode derivative of `raster`: out_dot = J . v for up to 16 tangents v of the inputs
(dpr_raster_jvp_ex_*, include/dpr.h "FORWARD-MODE DERIVATIVE").

For tangent k, pose b and point p, with the cell and deltas of `raster` held fixed (the one-sided derivative the
pullback uses, so J . v is the exact transpose of `raster_pullback_`):

    cdot_n    = n_n/2 * (Rdot[n, :] . p + R[n, :] . pdot + tdot[n])
    a         = owdot * pw + ow * pwdot
    b_n       = ow * pw * cdot_n
    out_dot[cell, k, b] = bgdot[k, b] + sum over (p, s) -> cell of a * voxel_weight(s) + sum_n b_n * interp_weight(n, s)

Tangents (all optional; None = zero):

  tangents=None  each tangent has its primal's shape (points_dot (P, N_in), rotation_dot (N_out, N_in) or
                 (B, N_out, N_in), translation_dot (N_out,) or (B, N_out), background_dot / out_weight_dot a scalar
                 or (B,), point_weight_dot (P,)) and out_dot has the shape and memory order of `raster`'s result
  tangents=K     each tangent has a leading axis of K (1..16) and out_dot is a K-plane image of logical shape
                 grid_size + (K,) [+ (B,)] with the memory of `empty_channel_grid(grid_size, K, B)`

The primal background does not enter; out_weight / point_weight None mean 1, as in `raster`.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import DimensionMismatch, _canonicalise, _image, _launch, _resolve, _workspace_bytes, empty_grid
from .channels import empty_channel_grid

MAX_TANGENTS = 16
_NAMES = ("points_dot", "rotation_dot", "translation_dot", "background_dot", "out_weight_dot", "point_weight_dot")


def _n_tangents(tangents):
    if tangents is None:
        return 1
    if isinstance(tangents, bool) or not isinstance(tangents, int) or not 1 <= tangents <= MAX_TANGENTS:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, f"tangents K = {tangents!r} out of range [1, {MAX_TANGENTS}]")
    return tangents


def resolve_algo_jvp(grid_size, n_points: int, batch: int, n_in: int, tangents: int = 1) -> str:
    """Name of the algorithm `algo="auto"` picks for a JVP call (dpr_resolve_algo_jvp)."""
    return _resolve("dpr_resolve_algo_jvp", (), grid_size, n_points, batch, n_in, tangents)


def workspace_bytes_jvp(grid_size, n_points: int, batch: int, n_in: int, tangents: int = 1, dtype=torch.float32,
                        algo: str = "auto") -> int:
    """dpr_workspace_bytes_jvp_ex_*: device bytes a JVP call needs."""
    return _workspace_bytes("_jvp", (_lib.ALGOS[algo], 0), dtype, grid_size, n_points, batch, n_in, tangents)


def _tangent(t, name, c, lead, shape, flat, scalar_ok=False):
    """The tangent as a contiguous buffer of shape `flat`, or None.  `lead` = () (tangents=None) or (K,)."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        if t.device != c["device"]:
            raise RuntimeError(f"{name} must be a tensor on the same HIP device as points (got {t.device})")
    elif scalar_ok:
        t = torch.as_tensor(t, dtype=torch.float64, device=c["device"])
    else:
        raise TypeError(f"{name} must be a torch.Tensor")
    want = lead + shape
    ok = tuple(t.shape) == want
    if not ok and scalar_ok and c["single"]:  # a single pose's scalar: () or (1,) per tangent
        ok = tuple(t.shape) in (lead, lead + (1,))
    if not ok:
        raise DimensionMismatch(f"size({name}) = {tuple(t.shape)} must be {want}")
    return t.to(c["dtype"]).reshape(flat).contiguous()


def raster_jvp_(out_dot, points, rotation, translation, background=None, out_weight=None, point_weight=None, *,
                points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None, out_weight_dot=None,
                point_weight_dot=None, tangents=None, algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place JVP: `out_dot` is overwritten and returned.  It has the shape of `raster`'s result (tangents=None)
    or grid_size + (K,) [+ (B,)] in the memory order of `empty_channel_grid` (tangents=K).  Enqueued on torch's
    current stream; not synchronised."""
    K = _n_tangents(tangents)
    c = _canonicalise(points, rotation, translation, background, out_weight, point_weight)
    P, B, n_in, n_out, single = c["P"], c["B"], c["n_in"], c["n_out"], c["single"]
    lead = () if tangents is None else (K,)
    pose = () if single else (B,)
    td = dict(
        points=_tangent(points_dot, "points_dot", c, lead, (P, n_in), (K, P, n_in)),
        rot=_tangent(rotation_dot, "rotation_dot", c, lead, pose + (n_out, n_in), (K, B, n_out, n_in)),
        trans=_tangent(translation_dot, "translation_dot", c, lead, pose + (n_out,), (K, B, n_out)),
        bg=_tangent(background_dot, "background_dot", c, lead, pose, (K, B), scalar_ok=True),
        ow=_tangent(out_weight_dot, "out_weight_dot", c, lead, pose, (K, B), scalar_ok=True),
        pw=_tangent(point_weight_dot, "point_weight_dot", c, lead, (P,), (K, P)),
    )
    if td["rot"] is not None:  # column-major per pose, as `rotation`
        td["rot"] = td["rot"].transpose(-1, -2).contiguous()
    _image(out_dot, "out_dot", c, [("tangents", k) for k in lead], out=True)
    _launch("_jvp", "dpr_raster_jvp_ex", None, c, out_dot.shape[:n_out], algo, 0, workspace, out_dot, c["points"],
            c["rot"], c["trans"], c["ow"], c["pw"], td["points"], td["rot"], td["trans"], td["bg"], td["ow"],
            td["pw"], tail=(K,))
    return out_dot


def raster_jvp(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None, *,
               points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None, out_weight_dot=None,
               point_weight_dot=None, tangents=None, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating JVP: the directional derivative of `raster(grid_size, points, ...)` along the given tangents."""
    K = _n_tangents(tangents)
    c = _canonicalise(points, rotation, translation, background, out_weight, point_weight)
    batch = None if c["single"] else c["B"]
    grid_size = tuple(int(n) for n in grid_size)
    if tangents is None:
        out_dot = empty_grid(grid_size, batch, c["dtype"], c["device"])
    else:
        out_dot = empty_channel_grid(grid_size, K, batch, c["dtype"], c["device"])
    return raster_jvp_(out_dot, points, rotation, translation, background, out_weight, point_weight,
                       points_dot=points_dot, rotation_dot=rotation_dot, translation_dot=translation_dot,
                       background_dot=background_dot, out_weight_dot=out_weight_dot,
                       point_weight_dot=point_weight_dot, tangents=tangents, algo=algo, workspace=workspace)
