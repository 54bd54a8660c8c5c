"""Point sampling: N-linear interpolation of images at the transformed points, forward and pullback
(dpr_sample_ex_* / dpr_sample_pullback_ex_*, include/dpr.h "SAMPLING").

For pose b

    values[p, b] = sum_s in-grid voxel_weight(deltas(R_b p + t_b), s) * image[ref(p, b) + shift_s, b]

with the cell choice, weights and drop rules of `raster` (0 for a rejected point): the transpose of `raster`
with respect to the point weights.  Shapes:

  image, ds_dimage   grid_size (single pose) or grid_size + (B,), in the memory order of `empty_grid`
                     (other layouts are copied with `to_grid_layout`)
  values, ds_dvalues (P,) single pose, (P, B) for a batch with the point index fastest (a transposed view of a
                     contiguous (B, P) tensor; `sample` allocates it that way)

Everything else is as for `raster`.  The pullback returns ds_dimage (`raster` of ds_dvalues[:, b] as point
weights, background 0, out_weight 1), ds_dpoints, ds_drotation and ds_dtranslation (the reference's
`raster_pullback!` terms with ds_dout = image_b, out_weight 1 and point weight ds_dvalues[:, b]).
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._args import (DimensionMismatch, _canonicalise, _cast_grads, _image, _launch, _op_code, _out_buf, _per_pose,
                    _resolve, _rotation_buf, _workspace_bytes)

SamplePullbackResult = namedtuple("SamplePullbackResult", ["image", "points", "rotation", "translation"])
_NAMES = SamplePullbackResult._fields
_ACCEPTED_OPS = ("raster", "sample", "pullback")


def resolve_algo_sample(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a sampling call (dpr_resolve_algo_sample);
    op is "sample" (or "raster") for the forward and "pullback"."""
    return _resolve("dpr_resolve_algo_sample", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch, n_in)


def workspace_bytes_sample(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                           algo: str = "auto") -> int:
    """dpr_workspace_bytes_sample_ex_*: device bytes a sampling call needs."""
    return _workspace_bytes("_sample", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in)


def _values_view(values, c, name):
    """(B, P) contiguous view of a (P,) / (P, B) point-fastest tensor (no copy)."""
    P, B = c["P"], c["B"]
    want = (P,) if c["single"] else (P, B)
    if not isinstance(values, torch.Tensor) or values.device != c["device"]:
        raise RuntimeError(f"{name} must be a tensor on the same HIP device as points")
    if tuple(values.shape) != want:
        raise DimensionMismatch(f"size({name}) = {tuple(values.shape)} must be {want}")
    return values.unsqueeze(0) if c["single"] else values.t()


def sample(image, points, rotation, translation, *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward: values (P,) for a single pose (rotation is a matrix), (P, B) with the point index
    fastest for a batch."""
    c = _canonicalise(points, rotation, translation, None, None, None, extra=(image,))
    P, B = c["P"], c["B"]
    if c["single"]:
        values = torch.empty((P,), dtype=c["dtype"], device=c["device"])
    else:
        values = torch.empty((B, P), dtype=c["dtype"], device=c["device"]).t()
    return sample_(values, image, points, rotation, translation, algo=algo, workspace=workspace)


def sample_(values, image, points, rotation, translation, *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place forward: `values` ((P,) or (P, B), point index fastest) is overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise(points, rotation, translation, None, None, None, extra=(image,))
    img = _image(image, "image", c)
    v = _values_view(values, c, "values")
    if values.dtype != c["dtype"]:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {c['dtype']}")
    if not v.is_contiguous():
        raise ValueError("values must have the point index fastest (a (P, B) transposed view of a (B, P) tensor)")
    _launch("_sample", "dpr_sample_ex", _lib.OP_RASTER, c, img.shape[: c["n_out"]], algo, 0, workspace,
            v, img, c["points"], c["rot"], c["trans"])
    return values


def sample_pullback_(ds_dvalues, image, points, rotation, translation, *, ds_dimage=None, ds_dpoints=None,
                     ds_drotation=None, ds_dtranslation=None, need=_NAMES, algo: str = "auto",
                     workspace=None) -> SamplePullbackResult:
    """Pullback of `sample`.  `need` names the gradients wanted (any of "image", "points", "rotation",
    "translation"); the others are neither computed nor written and come back as None.  Keyword outputs are
    pre-allocated buffers, OVERWRITTEN and returned by identity: ds_dimage in the grid layout of `empty_grid`,
    ds_dpoints (P, N_in), ds_drotation (B, N_out, N_in) as a transposed view of a contiguous (B, N_in, N_out)
    buffer (or (N_out, N_in) for a single pose), ds_dtranslation (B, N_out) (or (N_out,))."""
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
    c = _canonicalise(points, rotation, translation, None, None, None, extra=(image, ds_dvalues))
    P, B, n_in, n_out = c["P"], c["B"], c["n_in"], c["n_out"]
    img = _image(image, "image", c)
    dv = _values_view(ds_dvalues, c, "ds_dvalues").to(c["dtype"]).contiguous()
    d_img = d_pts = d_rot = d_trans = None
    if "image" in need:
        d_img = _out_buf(ds_dimage, img.shape, "ds_dimage", c, grid_layout=True)
    if "points" in need:
        d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    if "rotation" in need:
        d_rot = _rotation_buf(ds_drotation, c)
    if "translation" in need:
        d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=True)
    _launch("_sample", "dpr_sample_pullback_ex", _lib.OP_PULLBACK, c, img.shape[:n_out], algo, 0, workspace,
            dv, img, c["points"], c["rot"], c["trans"], d_img, d_pts, d_rot, d_trans)
    return SamplePullbackResult(d_img, d_pts, *_per_pose(c, d_rot, d_trans))


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, algo, image, points, rotation, translation):
        values = sample(image.detach(), points.detach(), rotation.detach(), translation.detach(),
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
        pb = sample_pullback_(ds_dvalues.detach(), image.detach(), points.detach(), rotation.detach(),
                              translation.detach(), need=need, algo=ctx.algo)
        return (None, *_cast_grads(want, pb, (image, points, rotation, translation)))


def sample_ad(image, points, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample` (torch autograd) with respect to image, points, rotation and translation
    (tensors); the tangents are those of `sample_pullback_`."""
    return _SampleFn.apply(algo, image, points, rotation, translation)
