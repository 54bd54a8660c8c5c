"""Forward-mode derivative of `raster_smooth_bodies`: out_dot = J . v for up to 16 tangents v of the inputs
(dpr_raster_smooth_bodies_jvp_ex_*, include/dpr.h "SMOOTH SPLAT, RIGID BODIES, FORWARD MODE").

K is the number of bodies, V the number of tangents.  With coord, j0, u, the weights w_d and their derivatives w'_d of
`raster_smooth` under pose (b, k), k = body[p], for tangent v, image b and an accepted point p:

    cdot_n     = n_n/2 * (Rdot[v, b, k][n, :] . p + R[b, k][n, :] . pdot[v, p] + tdot[v, b, k][n])
    a          = owdot[v, b] * pw[p] + ow[b] * pwdot[v, p],     c = ow[b] * pw[p]
    deposit(s) = a * prod_d w_d(s_d) + c * sum_n cdot_n * w'_n(s_n) * prod_{d != n} w_d(s_d)
    out_dot[j0 + s, v, b] = bgdot[v, b] + sum over (p, s) that land on the cell

No cell is held fixed: this is the exact directional derivative of `raster_smooth_bodies` and the exact transpose of
`raster_pullback_smooth_bodies_`.  A point that `raster_smooth_bodies` drops deposits nothing and none of its tangents
is read.  `body` has no tangent.

Tangents (all optional; None = zero):

  tangents=None  each tangent has its primal's shape (rotation_dot (B, K, N_out, N_in) or (K, N_out, N_in) for one
                 image, ...) and out_dot has the shape and memory order of `raster_smooth_bodies`' result
  tangents=V     each tangent has a leading axis of V (1..16): rotation_dot (V, B, K, N_out, N_in); out_dot is a
                 V-plane image of logical shape grid_size + (V,) [+ (B,)] with the memory of
                 `empty_channel_grid(grid_size, V, B)`

The shape errors and the `body` rules (int32 / int64, clamped narrowing) are those of the bodies family.  Algorithms:
"atomic", "tiled" (one binning per group of images serves all V tangents; `max_pose_group` bounds a group), "auto".
There is no public workspace query for this family, as for `raster_smooth_bodies`: every call asks
dpr_workspace_bytes_smooth_bodies_jvp_ex_* itself and allocates, or checks the `workspace` the caller passed (a uint8
tensor on the device); the C query is reachable through `lib()`.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import _image, _launch, _resolve, empty_grid
from .bodies import _canonicalise_bodies, _check_shapes
from .channels import empty_channel_grid
from .jvp import _n_tangents, _tangent


def resolve_algo_smooth_bodies_jvp(grid_size, n_points: int, batch: int, n_bodies: int, n_in: int,
                                   tangents: int = 1) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth rigid-body JVP call
    (dpr_resolve_algo_smooth_bodies_jvp)."""
    return _resolve("dpr_resolve_algo_smooth_bodies_jvp", (), grid_size, n_points, batch, n_in, n_bodies, tangents)


def raster_smooth_bodies_jvp_(out_dot, points, body, rotation, translation, background=None, out_weight=None,
                              point_weight=None, *, points_dot=None, rotation_dot=None, translation_dot=None,
                              background_dot=None, out_weight_dot=None, point_weight_dot=None, tangents=None,
                              algo: str = "auto", workspace=None, max_pose_group: int = 0) -> torch.Tensor:
    """In-place JVP: `out_dot` is overwritten and returned.  It has the shape of `raster_smooth_bodies`' result
    (tangents=None) or grid_size + (V,) [+ (B,)] in the memory order of `empty_channel_grid` (tangents=V).
    `max_pose_group` (1..16, 0 = default): the most images "tiled" bins together (DPR_FLAG_MAX_POSE_GROUP).  Enqueued
    on torch's current stream; not synchronised."""
    V = _n_tangents(tangents)
    _check_shapes(points, body, rotation, translation, point_weight)
    flags = _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything else)
    c = _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight)
    P, B, K, n_in, n_out, single = c["P"], c["B"], c["K"], c["n_in"], c["n_out"], c["single"]
    lead = () if tangents is None else (V,)
    pose = () if single else (B,)
    td = dict(
        points=_tangent(points_dot, "points_dot", c, lead, (P, n_in), (V, P, n_in)),
        rot=_tangent(rotation_dot, "rotation_dot", c, lead, pose + (K, n_out, n_in), (V, B * K, n_out, n_in)),
        trans=_tangent(translation_dot, "translation_dot", c, lead, pose + (K, n_out), (V, B * K, n_out)),
        bg=_tangent(background_dot, "background_dot", c, lead, pose, (V, B), scalar_ok=True),
        ow=_tangent(out_weight_dot, "out_weight_dot", c, lead, pose, (V, B), scalar_ok=True),
        pw=_tangent(point_weight_dot, "point_weight_dot", c, lead, (P,), (V, P)),
    )
    if td["rot"] is not None:  # column-major per pose, as `rotation`
        td["rot"] = td["rot"].transpose(-1, -2).contiguous()
    _image(out_dot, "out_dot", c, [("tangents", v) for v in lead], out=True)
    _launch("_smooth_bodies_jvp", "dpr_raster_smooth_bodies_jvp_ex", None, c, out_dot.shape[:n_out], algo, flags,
            workspace, out_dot, c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"], td["points"],
            td["rot"], td["trans"], td["bg"], td["ow"], td["pw"], tail=(K, V))
    return out_dot


def raster_smooth_bodies_jvp(grid_size, points, body, rotation, translation, background=None, out_weight=None,
                             point_weight=None, *, points_dot=None, rotation_dot=None, translation_dot=None,
                             background_dot=None, out_weight_dot=None, point_weight_dot=None, tangents=None,
                             algo: str = "auto", workspace=None, max_pose_group: int = 0) -> torch.Tensor:
    """Allocating JVP: the directional derivative of `raster_smooth_bodies(grid_size, points, body, ...)` along the
    tangents."""
    V = _n_tangents(tangents)
    _check_shapes(points, body, rotation, translation, point_weight)
    _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything is allocated)
    c = _canonicalise_bodies(points, body, rotation, translation, background, out_weight, point_weight)
    batch = None if c["single"] else c["B"]
    grid_size = tuple(int(n) for n in grid_size)
    if tangents is None:
        out_dot = empty_grid(grid_size, batch, c["dtype"], c["device"])
    else:
        out_dot = empty_channel_grid(grid_size, V, batch, c["dtype"], c["device"])
    return raster_smooth_bodies_jvp_(out_dot, points, body, rotation, translation, background, out_weight,
                                     point_weight, points_dot=points_dot, rotation_dot=rotation_dot,
                                     translation_dot=translation_dot, background_dot=background_dot,
                                     out_weight_dot=out_weight_dot, point_weight_dot=point_weight_dot,
                                     tangents=tangents, algo=algo, workspace=workspace,
                                     max_pose_group=max_pose_group)
