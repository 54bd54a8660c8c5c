"""Host-side mirror of the reference's public operator API for the hot path.

  raster(grid_size, points, rotation, translation[, background, out_weight, point_weight])
  raster_(out, ...)              == raster!            (/root/reference/src/interface.jl:48-55)
  raster_pullback_(ds_dout, ...) == raster_pullback!   (/root/reference/src/interface.jl:164-194)

Same argument meaning, defaults and error behaviour as the reference's dispatch
funnel (src/interface.jl:62-129, 196-308), with torch ROCm tensors as the device
arrays (the CuArray role in ext/DiffPointRasterisationCUDAExt.jl) and the C ABI of
include/dpr.h as the canonical methods (src/raster.jl:5-34,
ext/DiffPointRasterisationCUDAExt.jl:231-321).

Python-facing shapes are the mathematical ones; memory is the reference's:

  points        (P, N_in) contiguous                      Vector{SVector{N_in}}
  single pose:  rotation (N_out, N_in), translation (N_out,), background / out_weight scalars
  batched:      rotation (B, N_out, N_in), translation (B, N_out), background / out_weight (B,)
  out / ds_dout indexable as [i_1, .., i_N(, b)] like the reference's column-major arrays:
                a permuted view of a contiguous (B, n_N, .., n_1) buffer (`empty_grid`)

There is no CPU path: tensors must live on a HIP device and libdpr.so must be built.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import _lib
# (the funnel's public types and layouts are defined with it and are public here, as before)
from ._args import (ColumnMajorRotation, DimensionMismatch, column_major_rotation, empty_grid,  # noqa: F401
                    to_grid_layout)
from ._args import (_SUFFIX, _alloc_like, _as, _canonicalise, _device_of, _grid_call, _image, _launch, _op_code,
                    _out_buf, _per_pose, _ptr, _resolve, _rotation_buf, _stream_ptr, _workspace_bytes)

PullbackResult = namedtuple(
    "PullbackResult",
    ["points", "rotation", "translation", "background", "out_weight", "point_weight"],
)  # field order = src/raster_pullback.jl:74-81,140-147 (ChainRules slices it positionally)

_ACCEPTED_OPS = ("raster", "pullback", "residual_pullback")


def workspace_bytes(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                    algo: str = "auto", max_pose_group: int = 0,
                    coherent_points: bool = False, sharing: bool = False) -> int:
    """dpr_workspace_bytes_ex_*: device bytes `op` needs.  `max_pose_group` (1..16, 0 = default)
    bounds how many poses of a batch the tiled path bins together -- the speed / memory trade of
    DPR_FLAG_MAX_POSE_GROUP (include/dpr.h).  `sharing`: the calls will carry keep_binning /
    reuse_binning (`algo="auto"` then sizes for the algorithm the pair runs)."""
    flags = (_lib.flag_max_pose_group(max_pose_group)
             | (_lib.FLAG_COHERENT_POINTS if coherent_points else 0)
             | (_lib.FLAG_KEEP_BINNING if sharing else 0))
    return _workspace_bytes("", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], flags), dtype, grid_size,
                            n_points, batch, n_in)


def resolve_algo(op: str, grid_size, n_points: int, batch: int, n_in: int, *,
                 sharing: bool = False, coherent_points: bool = False) -> str:
    """Name of the algorithm `algo="auto"` picks for this problem.  `sharing`: the call carries
    keep_binning / reuse_binning (the choice is then made for the raster + pullback pair, see
    include/dpr.h)."""
    flags = (_lib.FLAG_KEEP_BINNING if sharing else 0) | (_lib.FLAG_COHERENT_POINTS if coherent_points else 0)
    return _resolve("dpr_resolve_algo_ex", (_op_code(op, _ACCEPTED_OPS), flags), grid_size, n_points, batch, n_in)


def sharing_effective(grid_size, n_points: int, batch: int, n_in: int, *,
                      coherent_points: bool = False) -> bool:
    """Will `algo="auto"` honour keep_binning / reuse_binning for this problem
    (dpr_resolve_flags_ex)?  False where the pair's algorithm has nothing to share."""
    flags = _lib.FLAG_KEEP_BINNING | (_lib.FLAG_COHERENT_POINTS if coherent_points else 0)
    rc = _grid_call(_lib.lib().dpr_resolve_flags_ex, (_lib.OP_RASTER, flags), n_in, grid_size, n_points, batch)
    if rc < 0:
        _lib.check(rc)
    return bool(rc & _lib.FLAG_KEEP_BINNING)


# --------------------------------------------------------------------------- forward
def raster(grid_size, points, rotation, translation, background=None, out_weight=None,
           point_weight=None, *, algo: str = "auto", workspace=None,
           max_pose_group: int = 0, coherent_points: bool = False) -> torch.Tensor:
    """Allocating forward (src/interface.jl:62-77).  Returns `out[i_1..i_N]` for a single
    pose (rotation is a matrix) or `out[i_1..i_N, b]` for a batch."""
    device, dtype, batch = _alloc_like(points, rotation, translation, background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), batch, dtype, device)
    return raster_(out, points, rotation, translation, background, out_weight, point_weight,
                   algo=algo, workspace=workspace, max_pose_group=max_pose_group,
                   coherent_points=coherent_points)


def raster_(out, points, rotation, translation, background=None, out_weight=None,
            point_weight=None, *, algo: str = "auto", workspace=None,
            keep_binning: bool = False, max_pose_group: int = 0,
            coherent_points: bool = False) -> torch.Tensor:
    """In-place forward, the reference's `raster!`.  `out` is fully overwritten and
    returned (same object).  Enqueued on torch's current stream; not synchronised.
    `keep_binning=True` (explicit `workspace`, sized with `sharing=True`) leaves the binning of
    every pose (tiled algorithm) or the sorted copy of the cloud (chunk-owner algorithm) in
    `workspace` for `raster_pullback_(..., reuse_binning=True)` with the same arguments."""
    c = _canonicalise(points, rotation, translation, background, out_weight, point_weight)
    _image(out, "out", c, out=True)
    flags = _lib.flag_max_pose_group(max_pose_group)
    flags |= _lib.FLAG_COHERENT_POINTS if coherent_points else 0  # dpr_sort_points output etc.
    flags |= _lib.FLAG_KEEP_BINNING if keep_binning else 0  # (also steers DPR_ALGO_AUTO)
    _launch("", "dpr_raster_ex", _lib.OP_RASTER, c, out.shape[: c["n_out"]], algo, flags, workspace,
            out, c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], refused_raises=True,
            workspace_required="keep_binning needs a caller-owned workspace" if keep_binning else None)
    return out


# --------------------------------------------------------------------------- pullback
def raster_pullback_(ds_dout, points, rotation, translation, background=None, out_weight=None,
                     point_weight=None, *, ds_dpoints=None, ds_drotation=None,
                     ds_dtranslation=None, ds_dbackground=None, ds_dout_weight=None,
                     ds_dpoint_weight=None, algo: str = "auto", workspace=None,
                     reuse_binning: bool = False, max_pose_group: int = 0,
                     coherent_points: bool = False,
                     point_weight_grad: bool = True) -> PullbackResult:
    """The reference's `raster_pullback!` (src/interface.jl:196-308).  Optional keyword
    arguments are pre-allocated outputs (the reference's `points=`, `rotation=`, ... kwargs,
    src/interface.jl:278-291); they are OVERWRITTEN and returned by identity.  Unlike the
    reference's GPU path (docs/src/batch.md:4) a single pose works too: scalars/unbatched
    arrays are returned for it as on the reference's CPU path (src/raster_pullback.jl:74-81).

    Returned layouts: points (P, N_in); rotation (B, N_out, N_in) -- a transposed view of
    the column-major (N_out, N_in, B) buffer; translation (B, N_out); background,
    out_weight (B,); point_weight (P,).

    `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither
    allocated nor written and comes back as None -- what the reference's rrule throws away
    when `point_weight` was defaulted (ext/DiffPointRasterisationChainRulesCoreExt.jl:23,70)."""
    return _pullback(ds_dout, None, points, rotation, translation, background, out_weight,
                     point_weight, ds_dpoints, ds_drotation, ds_dtranslation, ds_dbackground,
                     ds_dout_weight, ds_dpoint_weight, algo, workspace, reuse_binning,
                     max_pose_group, coherent_points, point_weight_grad)


def raster_residual_pullback_(out, target, points, rotation, translation, background=None,
                              out_weight=None, point_weight=None, *, scale: float = 2.0,
                              loss=None, ds_dpoints=None, ds_drotation=None,
                              ds_dtranslation=None, ds_dbackground=None, ds_dout_weight=None,
                              ds_dpoint_weight=None, algo: str = "auto", workspace=None,
                              reuse_binning: bool = False, coherent_points: bool = False):
    """Pullback of a squared-error loss without materialising its sensitivity
    (dpr_raster_residual_pullback_*).  Equivalent to

        ds_dout = scale * (out - target)          # README.md:151 (there: scale = -2)
        raster_pullback_(ds_dout, points, ...)     # src/interface.jl:196-308
        loss    = ((out - target) ** 2).sum over each pose's grid

    with `out` the result of `raster` for the same arguments; ds_dout is formed inside the
    kernels, so the grid is read once (out, target) instead of written and re-read.  Returns
    (PullbackResult, loss) with loss of shape (B,) (0-d for a single pose)."""
    return _pullback(out, (target, float(scale), loss), points, rotation, translation, background,
                     out_weight, point_weight, ds_dpoints, ds_drotation, ds_dtranslation,
                     ds_dbackground, ds_dout_weight, ds_dpoint_weight, algo, workspace,
                     reuse_binning, coherent_points=coherent_points)


def _pullback(ds_dout, residual, points, rotation, translation, background, out_weight,
              point_weight, ds_dpoints, ds_drotation, ds_dtranslation, ds_dbackground,
              ds_dout_weight, ds_dpoint_weight, algo, workspace, reuse_binning,
              max_pose_group=0, coherent_points=False, point_weight_grad=True):
    c = _canonicalise(points, rotation, translation, background, out_weight, point_weight,
                      extra=(ds_dout,))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    g = _image(ds_dout, "ds_dout", c)
    grid = g.shape[:n_out]
    tgt = None
    if residual is not None:
        target, res_scale, loss = residual
        tgt = _image(target, "target", c, grid=grid)
    d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    d_rot = _rotation_buf(ds_drotation, c)
    d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=True)
    d_bg = _out_buf(ds_dbackground, (B,), "ds_dbackground", c, reshape=True)
    d_ow = _out_buf(ds_dout_weight, (B,), "ds_dout_weight", c, reshape=True)
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = _out_buf(ds_dpoint_weight, (P,), "ds_dpoint_weight", c) if point_weight_grad else None
    d_loss = None if residual is None else _out_buf(loss, (B,), "loss", c, reshape=True)

    flags = _lib.flag_max_pose_group(max_pose_group)
    flags |= _lib.FLAG_COHERENT_POINTS if coherent_points else 0
    flags |= _lib.FLAG_REUSE_BINNING if reuse_binning else 0
    flags |= 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    pose = (c["points"], c["rot"], c["trans"], c["ow"], c["pw"])
    outs = (d_pts, d_rot, d_trans, d_bg, d_ow, d_pw)
    if residual is None:
        op, entry, args = _lib.OP_PULLBACK, "dpr_raster_pullback_ex", (g, *pose, *outs)
    else:
        op, entry, args = (_lib.OP_RESIDUAL_PULLBACK, "dpr_raster_residual_pullback_ex",
                           (g, tgt, res_scale, *pose, d_loss, *outs))
    _launch("", entry, op, c, grid, algo, flags, workspace, *args, refused_raises=True,
            workspace_required="reuse_binning needs the workspace of the preceding raster_ call"
            if reuse_binning else None)
    rot, trans, bg, ow, loss = _per_pose(c, d_rot, d_trans, d_bg, d_ow, d_loss)
    res = PullbackResult(d_pts, rot, trans, bg, ow, d_pw)
    return res if residual is None else (res, loss)


def sort_points(points: torch.Tensor, point_weight: Optional[torch.Tensor] = None):
    """Pose-independent Morton pre-sort of the model-frame points (dpr_sort_points_*).
    Returns (points_sorted, perm[, point_weight_sorted]) with points_sorted[i] =
    points[perm[i]]; gradients computed on the sorted cloud go back with
    `ds_dpoints.index_copy_(0, perm.long(), ds_dpoints_sorted)`."""
    device = _device_of(points)
    if points.ndim != 2 or points.dtype not in _SUFFIX:
        raise DimensionMismatch("points must be a (P, N_in) float32/float64 tensor")
    pts = points.contiguous()
    P, n_in = pts.shape
    out = torch.empty_like(pts)
    perm = torch.empty(P, dtype=torch.int32, device=device)
    pw = None if point_weight is None else _as(point_weight, pts.dtype, device, (P,), "point_weight")
    pw_out = None if pw is None else torch.empty_like(pw)
    L = _lib.lib()
    need = L.dpr_sort_points_workspace_bytes(P)
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        fn = getattr(L, f"dpr_sort_points_{_SUFFIX[pts.dtype]}")
        _lib.check(fn(_stream_ptr(device), n_in, P, _ptr(pts), _ptr(out), _ptr(perm), _ptr(pw),
                      _ptr(pw_out), _ptr(ws), ws.numel()))
    return (out, perm) if pw is None else (out, perm, pw_out)
