"""Forward-mode derivative of `raster_smooth`: out_dot = J . v for up to 16 tangents v of the inputs
(dpr_raster_smooth_jvp_ex_*, include/dpr.h "SMOOTH SPLAT, FORWARD MODE").

With coord, j0, u, the weights w_d and their derivatives w'_d of `raster_smooth`, for tangent k, pose b and an
accepted point p:

    cdot_n     = n_n/2 * (Rdot[n, :] . p + R[n, :] . pdot + tdot[n])
    a          = owdot * pw + ow * pwdot,     c = ow * pw
    deposit(s) = a * prod_d w_d(s_d) + c * sum_n cdot_n * w'_n(s_n) * prod_{d != n} w_d(s_d)
    out_dot[j0 + s, k, b] = bgdot[k, b] + sum over (p, s) that land on the cell

No cell is held fixed: `raster_smooth` is C1, so this is its exact directional derivative, continuous across cell
faces, and the exact transpose of `raster_pullback_smooth_`.  The keyword tangents, `tangents=None | K`, the shape
errors and the output shapes are those of `raster_jvp` / `raster_jvp_`; (N_in, N_out): (2,2), (3,3), (3,2).
Algorithms: "atomic", "tiled" (one binning per pose serves all K tangents), "auto".
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import _image, _launch, _resolve, _workspace_bytes, empty_grid
from .channels import empty_channel_grid
from .jvp import _n_tangents, _tangent
from .smooth import _canonicalise_smooth


def resolve_algo_smooth_jvp(grid_size, n_points: int, batch: int, n_in: int, tangents: int = 1) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth JVP call (dpr_resolve_algo_smooth_jvp)."""
    return _resolve("dpr_resolve_algo_smooth_jvp", (), grid_size, n_points, batch, n_in, tangents)


def workspace_bytes_smooth_jvp(grid_size, n_points: int, batch: int, n_in: int, tangents: int = 1,
                               dtype=torch.float32, algo: str = "auto") -> int:
    """dpr_workspace_bytes_smooth_jvp_ex_*: device bytes a smooth JVP call needs."""
    return _workspace_bytes("_smooth_jvp", (_lib.ALGOS[algo], 0), dtype, grid_size, n_points, batch, n_in, tangents)


def raster_smooth_jvp_(out_dot, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                       *, points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None,
                       out_weight_dot=None, point_weight_dot=None, tangents=None, algo: str = "auto",
                       workspace=None) -> torch.Tensor:
    """In-place JVP: `out_dot` is overwritten and returned.  It has the shape of `raster_smooth`'s result
    (tangents=None) or grid_size + (K,) [+ (B,)] in the memory order of `empty_channel_grid` (tangents=K).
    Enqueued on torch's current stream; not synchronised."""
    K = _n_tangents(tangents)
    c = _canonicalise_smooth(points, rotation, translation, background, out_weight, point_weight)
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
    _launch("_smooth_jvp", "dpr_raster_smooth_jvp_ex", None, c, out_dot.shape[:n_out], algo, 0, workspace, out_dot,
            c["points"], c["rot"], c["trans"], c["ow"], c["pw"], td["points"], td["rot"], td["trans"], td["bg"],
            td["ow"], td["pw"], tail=(K,))
    return out_dot


def raster_smooth_jvp(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                      *, points_dot=None, rotation_dot=None, translation_dot=None, background_dot=None,
                      out_weight_dot=None, point_weight_dot=None, tangents=None, algo: str = "auto",
                      workspace=None) -> torch.Tensor:
    """Allocating JVP: the directional derivative of `raster_smooth(grid_size, points, ...)` along the tangents."""
    K = _n_tangents(tangents)
    c = _canonicalise_smooth(points, rotation, translation, background, out_weight, point_weight)
    batch = None if c["single"] else c["B"]
    grid_size = tuple(int(n) for n in grid_size)
    if tangents is None:
        out_dot = empty_grid(grid_size, batch, c["dtype"], c["device"])
    else:
        out_dot = empty_channel_grid(grid_size, K, batch, c["dtype"], c["device"])
    return raster_smooth_jvp_(out_dot, points, rotation, translation, background, out_weight, point_weight,
                              points_dot=points_dot, rotation_dot=rotation_dot, translation_dot=translation_dot,
                              background_dot=background_dot, out_weight_dot=out_weight_dot,
                              point_weight_dot=point_weight_dot, tangents=tangents, algo=algo, workspace=workspace)
