"""Smooth sampling of C-channel images: `sample_smooth` of every plane of a (grid..., C[, B]) image at the transformed
points, forward and pullback (dpr_sample_smooth_channels_ex_* / dpr_sample_smooth_channels_pullback_ex_*,
include/dpr.h "SMOOTH SAMPLING, MULTI-CHANNEL").

    values[p, c, b] = sum_s in-grid image[j0 + s, c, b] * prod_d w_d(s_d),   s in {-1, 0, +1}^N_out

(0 for a rejected point) with the cell and the weights of `raster_smooth` under pose b: C features per point, C1 in
the point position -- what `torch.nn.functional.grid_sample` is to a feature map, with the exact gradient in the
image, the points and the poses.  `values[:, c, b]` is `sample_smooth` of plane (c, b), bit for bit; the cell, the
weights and the offsets of a (point, pose) are computed once for the C channels.  The operator is the transpose of
`raster_smooth_channels` in the point weights, with one weight per (point, channel, pose).

Shapes and memory:

  image, ds_dimage     grid_size + (C,) [+ (B,)]   what `raster_smooth_channels` returns; `empty_channel_grid`
  values, ds_dvalues   (P, C) single pose          a point's C values contiguous
                       (P, C, B)                   the view `.permute(1, 2, 0)` of a contiguous (B, P, C) tensor, so
                                                   that `ds_dvalues[..., b]` is a point_weight of `raster_smooth_channels`

C = 1..16 is read from the image, or from ds_dvalues where there is no image.  (N_in, N_out): (2,2), (3,3), (3,2).
Algorithms: "atomic" (forward and pullback), "tiled" (pullback: ds_dimage through the tiled `raster_smooth_channels`,
one binning per pose for all C channels), "auto".  There is no public workspace query for this family: every call
asks dpr_workspace_bytes_sample_smooth_channels_ex_* itself and allocates, or checks the `workspace` the caller passed
(a uint8 tensor on the device); the C query is reachable through `lib()`.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (DimensionMismatch, _cast_grads, _image, _launch, _op_code, _out_buf, _per_pose, _resolve,
                    _rotation_buf)
from .channels import _check_channels
from .sample import SamplePullbackResult
from .smooth import _canonicalise_smooth

_NAMES = SamplePullbackResult._fields
_ACCEPTED_OPS = ("raster", "sample", "pullback")
_FAMILY = "_sample_smooth_channels"


def resolve_algo_sample_smooth_channels(op: str, grid_size, n_points: int, batch: int, n_in: int,
                                        channels: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a call (dpr_resolve_algo_sample_smooth_channels); op is
    "sample" (or "raster") for the forward and "pullback"."""
    return _resolve("dpr_resolve_algo_sample_smooth_channels", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points,
                    batch, n_in, channels)


def _image_channels(image, c, name="image"):
    """C of an image-shaped tensor of the canonical call `c` (its axis after the grid)."""
    n_out = c["n_out"]
    want = n_out + (1 if c["single"] else 2)
    if not isinstance(image, torch.Tensor) or image.ndim != want:
        nd = image.ndim if isinstance(image, torch.Tensor) else type(image).__name__
        raise DimensionMismatch(f"{name} has {nd} dims, expected {want}: grid_size + (C,)"
                                f"{'' if c['single'] else ' + (B,)'} for N_out={n_out}")
    C = int(image.shape[n_out])
    _check_channels(C)
    return C


def _values_view(values, c, C, name):
    """(B, P, C) view of a (P, C) / (P, C, B) tensor (no copy); C is checked against `C` unless that is None."""
    P, B = c["P"], c["B"]
    if not isinstance(values, torch.Tensor) or values.device != c["device"]:
        raise RuntimeError(f"{name} must be a tensor on the same HIP device as points")
    nd = 2 if c["single"] else 3
    shape = tuple(values.shape)
    if C is None and len(shape) == nd:
        C = int(shape[1])
    want = (P, C) if c["single"] else (P, C, B)
    if shape != want:
        raise DimensionMismatch(f"size({name}) = {shape} must be {want} "
                                f"((n_points, C){'' if c['single'] else ' + (B,)'})")
    _check_channels(C)
    return (values.unsqueeze(0) if c["single"] else values.permute(2, 0, 1)), C


def sample_smooth_channels(image, points, rotation, translation, *, algo: str = "auto",
                           workspace=None) -> torch.Tensor:
    """Allocating forward: values (P, C) for a single pose (rotation is a matrix), (P, C, B) -- a view of a
    contiguous (B, P, C) tensor -- for a batch."""
    c = _canonicalise_smooth(points, rotation, translation, None, None, None, extra=(image,))
    P, B = c["P"], c["B"]
    C = _image_channels(image, c)
    if c["single"]:
        values = torch.empty((P, C), dtype=c["dtype"], device=c["device"])
    else:
        values = torch.empty((B, P, C), dtype=c["dtype"], device=c["device"]).permute(1, 2, 0)
    return sample_smooth_channels_(values, image, points, rotation, translation, algo=algo, workspace=workspace)


def sample_smooth_channels_(values, image, points, rotation, translation, *, algo: str = "auto",
                            workspace=None) -> torch.Tensor:
    """In-place forward: `values` ((P, C), or the (P, C, B) view of a contiguous (B, P, C) tensor) is overwritten
    and returned.  Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_smooth(points, rotation, translation, None, None, None, extra=(image,))
    C = _image_channels(image, c)
    img = _image(image, "image", c, (("channels", C),))
    v, _ = _values_view(values, c, C, "values")
    if values.dtype != c["dtype"]:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {c['dtype']}")
    if not v.is_contiguous():
        raise ValueError("values must have a point's C values contiguous and the pose slowest "
                         "(a (P, C, B) permuted view of a contiguous (B, P, C) tensor)")
    _launch(_FAMILY, "dpr_sample_smooth_channels_ex", _lib.OP_RASTER, c, img.shape[: c["n_out"]], algo, 0, workspace,
            v, img, c["points"], c["rot"], c["trans"], tail=(C,))
    return values


def sample_smooth_channels_pullback_(ds_dvalues, image, points, rotation, translation, *, ds_dimage=None,
                                     ds_dpoints=None, ds_drotation=None, ds_dtranslation=None, need=_NAMES,
                                     algo: str = "auto", workspace=None, grid_size=None,
                                     channels=None) -> SamplePullbackResult:
    """Pullback of `sample_smooth_channels`.  `need` names the gradients wanted (any of "image", "points",
    "rotation", "translation"); the others are neither computed nor written and come back as None.  Keyword outputs
    are pre-allocated buffers, OVERWRITTEN and returned by identity: ds_dimage shaped like image (the memory of
    `empty_channel_grid`), the others as for `sample_smooth_pullback_`.  ds_dpoints, ds_drotation and ds_dtranslation
    are sums over the channels.
    `image` may be None when only "image" is needed (ds_dimage does not depend on it); the grid then comes from the
    ds_dimage buffer or from `grid_size`, and C from ds_dvalues.  `channels`, where given, must be that C."""
    need = tuple(need)
    for n in need:
        if n not in _NAMES:
            raise ValueError(f"need: unknown gradient {n!r} (choose from {_NAMES})")
    if not need:
        raise ValueError("need: at least one gradient must be wanted")
    given = dict(image=ds_dimage, points=ds_dpoints, rotation=ds_drotation, translation=ds_dtranslation)
    for n, buf in given.items():
        if buf is not None and n not in need:
            raise ValueError(f"a ds_d{n} buffer was given but {n!r} is not in need")
    c = _canonicalise_smooth(points, rotation, translation, None, None, None, extra=(image, ds_dvalues))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    C = None if channels is None else int(channels)
    if image is None:
        if need != ("image",):
            raise ValueError("image=None: only ds_dimage can be computed without the image (need=('image',))")
        if ds_dimage is None and grid_size is None:
            raise ValueError("image=None: pass a ds_dimage buffer or grid_size")
        img = None
        grid = tuple(ds_dimage.shape[:n_out]) if grid_size is None else tuple(int(n) for n in grid_size)
    else:
        Ci = _image_channels(image, c)
        if C is not None and C != Ci:
            raise DimensionMismatch(f"channels = {C} but the image has {Ci}")
        C = Ci
        img = _image(image, "image", c, (("channels", C),), grid=grid_size)
        grid = tuple(img.shape[:n_out])
    dv, C = _values_view(ds_dvalues, c, C, "ds_dvalues")
    dv = dv.to(c["dtype"]).contiguous()
    d_img = d_pts = d_rot = d_trans = None
    if "image" in need:
        d_img = _out_buf(ds_dimage, grid + (C,) + (() if c["single"] else (B,)), "ds_dimage", c, grid_layout=True)
    if "points" in need:
        d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    if "rotation" in need:
        d_rot = _rotation_buf(ds_drotation, c)
    if "translation" in need:
        d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=True)
    _launch(_FAMILY, "dpr_sample_smooth_channels_pullback_ex", _lib.OP_PULLBACK, c, grid, algo, 0, workspace,
            dv, img, c["points"], c["rot"], c["trans"], d_img, d_pts, d_rot, d_trans, tail=(C,))
    return SamplePullbackResult(d_img, d_pts, *_per_pose(c, d_rot, d_trans))


class _SampleSmoothChannelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, algo, image, points, rotation, translation):
        values = sample_smooth_channels(image.detach(), points.detach(), rotation.detach(), translation.detach(),
                                        algo="atomic" if algo == "tiled" else algo)  # (no tiled forward)
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
        pb = sample_smooth_channels_pullback_(ds_dvalues.detach(), image.detach(), points.detach(),
                                              rotation.detach(), translation.detach(), need=need, algo=ctx.algo)
        return (None, *_cast_grads(want, pb, (image, points, rotation, translation)))


def sample_smooth_channels_ad(image, points, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample_smooth_channels` (torch autograd) with respect to image, points, rotation and
    translation (tensors); the tangents are those of `sample_smooth_channels_pullback_`."""
    return _SampleSmoothChannelsFn.apply(algo, image, points, rotation, translation)
