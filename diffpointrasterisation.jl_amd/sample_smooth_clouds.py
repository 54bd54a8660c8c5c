"""Smooth sampling at per-pose point clouds: `sample_smooth` with a different cloud for every pose, forward and
pullback (dpr_sample_smooth_clouds_ex_* / dpr_sample_smooth_clouds_pullback_ex_*, include/dpr.h "SMOOTH SAMPLING,
PER-POSE CLOUDS").  The direction `raster_smooth_clouds` lacks: image b read back at cloud b.

For pose b, with its own cloud points[b]:

    values[b, p] = sum_s in-grid image[j0 + s, b] * prod_d w_d(s_d)   at R_b points[b, p] + t_b,  s in {-1, 0, +1}^N_out

(0 for a point `raster_smooth` would drop; NaN coordinates are dropped too).  Row b is exactly
`sample_smooth(image[..., b], points[b], R_b, t_b)`, bit for bit, and the pullback decomposes the same way
(ds_dpoints[b] is the single-pose gradient of pose b: no sum over poses).  One call in the place of a Python loop of
B single-pose calls; on "tiled" the pullback's ds_dimage bins the poses in groups, four launches per group instead
of four per pose.  Shapes:

  points, ds_dpoints       (B, P, N_in) contiguous
  values, ds_dvalues       (B, P) contiguous -- the pose first, as everywhere in the clouds family (not the (P, B)
                           transposed view of `sample_smooth`); the layout of point_weight of `raster_smooth_clouds`
  image, ds_dimage         grid_size + (B,) in the memory order of `empty_grid`
  rotation, translation    batched: (B, N_out, N_in), (B, N_out)

(N_in, N_out): (2,2), (3,3), (3,2).  Algorithms: "atomic" (forward and pullback), "tiled" (pullback), "auto".

Clouds of different sizes: pad them to a common P.  The values of the padded points are to be ignored and their
ds_dvalues set to 0, which gives them zero gradients and no deposit in ds_dimage.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (ColumnMajorRotation, DimensionMismatch, _cast_grads, _image, _launch, _op_code, _out_buf,
                    _promote, _resolve, _rotation_buf, _workspace_bytes)
from .clouds import _canonicalise_clouds
from .clouds import _check_shapes as _check_cloud_shapes
from .sample import SamplePullbackResult
from .smooth import _PAIRS

_NAMES = SamplePullbackResult._fields
_ACCEPTED_OPS = ("raster", "sample", "pullback")


def resolve_algo_sample_smooth_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a call (dpr_resolve_algo_sample_smooth_clouds); op is "sample"
    (or "raster") for the forward and "pullback"; n_points is P, the points of each cloud."""
    return _resolve("dpr_resolve_algo_sample_smooth_clouds", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points,
                    batch, n_in)


def workspace_bytes_sample_smooth_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int,
                                         dtype=torch.float32, algo: str = "auto", max_pose_group: int = 0) -> int:
    """dpr_workspace_bytes_sample_smooth_clouds_ex_*: device bytes a call needs (none off the "tiled" pullback, where
    it is `workspace_bytes_smooth_clouds("raster", ..., algo="tiled", max_pose_group=...)`).  `max_pose_group` (1..16,
    0 = default) must be the value the call itself will carry.  An attribute of the package and of this module, not
    of the package's `__all__`."""
    return _workspace_bytes("_sample_smooth_clouds", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo],
                                                      _lib.flag_max_pose_group(max_pose_group)),
                            dtype, grid_size, n_points, batch, n_in)


def _check_shapes(points, rotation, translation):
    """The shape and dimension errors of a call, raised before anything else looks at the arguments (and before any
    library call): those of per-pose clouds, then the (N_in, N_out) pairs the smooth splat has."""
    _check_cloud_shapes(points, rotation, translation, None)
    rs = tuple(rotation.shape) if isinstance(rotation, (torch.Tensor, ColumnMajorRotation)) \
        else tuple(torch.as_tensor(rotation).shape)
    if (rs[2], rs[1]) not in _PAIRS:
        raise DimensionMismatch(f"sample_smooth_clouds supports (N_in, N_out) in {_PAIRS}, got {(rs[2], rs[1])}")


def _check_values(t, name, points):
    """values / ds_dvalues against the clouds: a (B, P) tensor."""
    B, P = points.shape[0], points.shape[1]
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if tuple(t.shape) != (B, P):
        raise DimensionMismatch(f"{name} must be (B, P) = {(B, P)}, got {tuple(t.shape)}")


def _check_need(need, given):
    need = tuple(need)
    for n in need:
        if n not in _NAMES:
            raise ValueError(f"need: unknown gradient {n!r} (choose from {_NAMES})")
    if not need:
        raise ValueError("need: at least one gradient must be wanted")
    for n, buf in given.items():
        if buf is not None and n not in need:
            raise ValueError(f"a ds_d{n} buffer was given but {n!r} is not in need")
    return need


def sample_smooth_clouds(image, points, rotation, translation, *, algo: str = "auto", workspace=None,
                         max_pose_group: int = 0) -> torch.Tensor:
    """Allocating forward: returns values (B, P), contiguous."""
    _check_shapes(points, rotation, translation)
    _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything is allocated)
    c = _canonicalise_clouds(points, rotation, translation, None, None, None, extra=(image,))
    values = torch.empty((c["B"], c["P"]), dtype=c["dtype"], device=c["device"])
    return sample_smooth_clouds_(values, image, points, rotation, translation, algo=algo, workspace=workspace,
                                 max_pose_group=max_pose_group)


def sample_smooth_clouds_(values, image, points, rotation, translation, *, algo: str = "auto", workspace=None,
                          max_pose_group: int = 0) -> torch.Tensor:
    """In-place forward: `values` ((B, P), contiguous) is overwritten and returned.  `max_pose_group` is accepted
    for symmetry with the pullback and ignored (the forward forms no groups).  Enqueued on torch's current stream;
    not synchronised."""
    _check_shapes(points, rotation, translation)
    _check_values(values, "values", points)
    flags = _lib.flag_max_pose_group(max_pose_group)
    dtype = _promote(points, rotation.cm if isinstance(rotation, ColumnMajorRotation) else rotation, translation,
                     image)
    if values.dtype != dtype:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {dtype}")
    c = _canonicalise_clouds(points, rotation, translation, None, None, None, extra=(image,))
    img = _image(image, "image", c)
    if values.device != c["device"] or not values.is_contiguous():
        raise ValueError("values must be a contiguous (B, P) tensor on the device of points")
    _launch("_sample_smooth_clouds", "dpr_sample_smooth_clouds_ex", _lib.OP_RASTER, c, img.shape[: c["n_out"]], algo,
            flags, workspace, values, img, c["points"], c["rot"], c["trans"])
    return values


def sample_smooth_clouds_pullback_(ds_dvalues, image, points, rotation, translation, *, ds_dimage=None,
                                   ds_dpoints=None, ds_drotation=None, ds_dtranslation=None, need=_NAMES,
                                   algo: str = "auto", workspace=None, grid_size=None,
                                   max_pose_group: int = 0) -> SamplePullbackResult:
    """Pullback of `sample_smooth_clouds`.  `need` names the gradients wanted (any of "image", "points", "rotation",
    "translation"); the others are neither computed nor written and come back as None.  Keyword outputs are
    pre-allocated buffers, OVERWRITTEN and returned by identity: ds_dimage grid_size + (B,) in the memory order of
    `empty_grid`; ds_dpoints (B, P, N_in); ds_drotation (B, N_out, N_in) as a transposed view of a contiguous
    (B, N_in, N_out) buffer; ds_dtranslation (B, N_out).  `image` may be None when only "image" is needed (ds_dimage
    does not depend on it); the grid then comes from the ds_dimage buffer or from `grid_size`.  `max_pose_group`
    (1..16, 0 = default): the most poses the "tiled" ds_dimage bins together (DPR_FLAG_MAX_POSE_GROUP)."""
    need = _check_need(need, dict(image=ds_dimage, points=ds_dpoints, rotation=ds_drotation,
                                  translation=ds_dtranslation))
    _check_shapes(points, rotation, translation)
    _check_values(ds_dvalues, "ds_dvalues", points)
    flags = _lib.flag_max_pose_group(max_pose_group)
    if image is None:
        if need != ("image",):
            raise ValueError("image=None: only ds_dimage can be computed without the image (need=('image',))")
        if ds_dimage is None and grid_size is None:
            raise ValueError("image=None: pass a ds_dimage buffer or grid_size")
    c = _canonicalise_clouds(points, rotation, translation, None, None, None, extra=(image, ds_dvalues))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    if image is None:
        img = None
        grid = tuple(ds_dimage.shape[:n_out]) if grid_size is None else tuple(int(n) for n in grid_size)
    else:
        img = _image(image, "image", c, grid=grid_size)
        grid = tuple(img.shape[:n_out])
    dv = ds_dvalues.to(device=c["device"], dtype=c["dtype"]).contiguous()
    d_img = d_pts = d_rot = d_trans = None
    if "image" in need:
        d_img = _out_buf(ds_dimage, grid + (B,), "ds_dimage", c, grid_layout=True)
    if "points" in need:
        d_pts = _out_buf(ds_dpoints, (B, P, n_in), "ds_dpoints", c)
    if "rotation" in need:
        d_rot = _rotation_buf(ds_drotation, c)
    if "translation" in need:
        d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c)
    # (without poses every output is empty -- as ds_dpoints alone is without points -- and an empty tensor has no
    # pointer to pass: the library would see a call that wants nothing)
    if any(t is not None and t.numel() > 0 for t in (d_img, d_pts, d_rot, d_trans)):
        _launch("_sample_smooth_clouds", "dpr_sample_smooth_clouds_pullback_ex", _lib.OP_PULLBACK, c, grid, algo,
                flags, workspace, dv, img, c["points"], c["rot"], c["trans"], d_img, d_pts, d_rot, d_trans)
    return SamplePullbackResult(d_img, d_pts, None if d_rot is None else d_rot.transpose(1, 2), d_trans)


class _SampleSmoothCloudsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, algo, image, points, rotation, translation):
        values = sample_smooth_clouds(image.detach(), points.detach(), rotation.detach(), translation.detach(),
                                      algo="atomic" if algo == "tiled" else algo)  # (the forward has no tiled variant)
        ctx.save_for_backward(image, points, rotation, translation)
        ctx.algo = algo
        return values

    @staticmethod
    def backward(ctx, ds_dvalues):
        image, points, rotation, translation = ctx.saved_tensors
        want = ctx.needs_input_grad[1:]  # (image, points, rotation, translation)
        need = tuple(n for n, w in zip(_NAMES, want) if w)
        if not need:
            return None, None, None, None, None
        pb = sample_smooth_clouds_pullback_(ds_dvalues.detach(), image.detach(), points.detach(), rotation.detach(),
                                            translation.detach(), need=need, algo=ctx.algo)
        return (None, *_cast_grads(want, pb, (image, points, rotation, translation)))


def sample_smooth_clouds_ad(image, points, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample_smooth_clouds` (torch autograd) with respect to image, points, rotation and
    translation (tensors); the tangents are those of `sample_smooth_clouds_pullback_`.  A forward on "tiled" runs
    "atomic"."""
    return _SampleSmoothCloudsFn.apply(algo, image, points, rotation, translation)
