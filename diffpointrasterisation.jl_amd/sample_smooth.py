"""Smooth point sampling: quadratic B-spline interpolation of images at the transformed points, forward and
pullback (dpr_sample_smooth_ex_* / dpr_sample_smooth_pullback_ex_*, include/dpr.h "SMOOTH SAMPLING").

`sample` interpolates N-linearly: its gradient with respect to the points is piecewise constant per cell.
`sample_smooth` reads the image with the weights `raster_smooth` deposits with,

    values[p, b] = sum_s in-grid image[j0 + s, b] * prod_d w_d(s_d),   s in {-1, 0, +1}^N_out

(0 for a rejected point): C1 in the point position, the transpose of `raster_smooth` with respect to the point
weights.  Shapes and layouts are those of `sample`: image / ds_dimage grid_size (single pose) or grid_size + (B,)
in the memory order of `empty_grid`; values / ds_dvalues (P,) or (P, B) with the point index fastest.
(N_in, N_out): (2,2), (3,3), (3,2).  Algorithms: "atomic" (forward and pullback), "tiled" (pullback), "auto".

The pullback returns ds_dimage (`raster_smooth` of ds_dvalues[:, b] as point weights, background 0, out_weight 1)
and the exact derivatives ds_dpoints, ds_drotation and ds_dtranslation (`raster_pullback_smooth_`'s terms with
ds_dout = image_b, out_weight 1 and point weight ds_dvalues[:, b]).
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import (_cast_grads, _image, _launch, _op_code, _out_buf, _per_pose, _resolve, _rotation_buf,
                    _workspace_bytes)
from .sample import SamplePullbackResult, _values_view
from .smooth import _canonicalise_smooth

_NAMES = SamplePullbackResult._fields
_ACCEPTED_OPS = ("raster", "sample", "pullback")


def resolve_algo_sample_smooth(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a smooth sampling call (dpr_resolve_algo_sample_smooth);
    op is "sample" (or "raster") for the forward and "pullback"."""
    return _resolve("dpr_resolve_algo_sample_smooth", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points, batch,
                    n_in)


def workspace_bytes_sample_smooth(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                                  algo: str = "auto") -> int:
    """dpr_workspace_bytes_sample_smooth_ex_*: device bytes a smooth sampling call needs."""
    return _workspace_bytes("_sample_smooth", (_op_code(op, _ACCEPTED_OPS), _lib.ALGOS[algo], 0), dtype, grid_size,
                            n_points, batch, n_in)


def sample_smooth(image, points, rotation, translation, *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward: values (P,) for a single pose (rotation is a matrix), (P, B) with the point index
    fastest for a batch."""
    c = _canonicalise_smooth(points, rotation, translation, None, None, None, extra=(image,))
    P, B = c["P"], c["B"]
    if c["single"]:
        values = torch.empty((P,), dtype=c["dtype"], device=c["device"])
    else:
        values = torch.empty((B, P), dtype=c["dtype"], device=c["device"]).t()
    return sample_smooth_(values, image, points, rotation, translation, algo=algo, workspace=workspace)


def sample_smooth_(values, image, points, rotation, translation, *, algo: str = "auto",
                   workspace=None) -> torch.Tensor:
    """In-place forward: `values` ((P,) or (P, B), point index fastest) is overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_smooth(points, rotation, translation, None, None, None, extra=(image,))
    img = _image(image, "image", c)
    v = _values_view(values, c, "values")
    if values.dtype != c["dtype"]:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {c['dtype']}")
    if not v.is_contiguous():
        raise ValueError("values must have the point index fastest (a (P, B) transposed view of a (B, P) tensor)")
    _launch("_sample_smooth", "dpr_sample_smooth_ex", _lib.OP_RASTER, c, img.shape[: c["n_out"]], algo, 0, workspace,
            v, img, c["points"], c["rot"], c["trans"])
    return values


def sample_smooth_pullback_(ds_dvalues, image, points, rotation, translation, *, ds_dimage=None, ds_dpoints=None,
                            ds_drotation=None, ds_dtranslation=None, need=_NAMES, algo: str = "auto",
                            workspace=None, grid_size=None) -> SamplePullbackResult:
    """Pullback of `sample_smooth`.  `need` names the gradients wanted (any of "image", "points", "rotation",
    "translation"); the others are neither computed nor written and come back as None.  Keyword outputs are
    pre-allocated buffers, OVERWRITTEN and returned by identity, with the shapes of `sample_pullback_`.
    `image` may be None when only "image" is needed (ds_dimage does not depend on it); the grid then comes from
    the ds_dimage buffer or from `grid_size`."""
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
    if image is None:
        if need != ("image",):
            raise ValueError("image=None: only ds_dimage can be computed without the image (need=('image',))")
        if ds_dimage is None and grid_size is None:
            raise ValueError("image=None: pass a ds_dimage buffer or grid_size")
        img = None
        grid = tuple(ds_dimage.shape[:n_out]) if grid_size is None else tuple(int(n) for n in grid_size)
    else:
        img = _image(image, "image", c, grid=grid_size)
        grid = tuple(img.shape[:n_out])
    dv = _values_view(ds_dvalues, c, "ds_dvalues").to(c["dtype"]).contiguous()
    d_img = d_pts = d_rot = d_trans = None
    if "image" in need:
        d_img = _out_buf(ds_dimage, grid + (() if c["single"] else (B,)), "ds_dimage", c, grid_layout=True)
    if "points" in need:
        d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    if "rotation" in need:
        d_rot = _rotation_buf(ds_drotation, c)
    if "translation" in need:
        d_trans = _out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation", c, reshape=True)
    _launch("_sample_smooth", "dpr_sample_smooth_pullback_ex", _lib.OP_PULLBACK, c, grid, algo, 0, workspace,
            dv, img, c["points"], c["rot"], c["trans"], d_img, d_pts, d_rot, d_trans)
    return SamplePullbackResult(d_img, d_pts, *_per_pose(c, d_rot, d_trans))


class _SampleSmoothFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, algo, image, points, rotation, translation):
        values = sample_smooth(image.detach(), points.detach(), rotation.detach(), translation.detach(),
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
        pb = sample_smooth_pullback_(ds_dvalues.detach(), image.detach(), points.detach(), rotation.detach(),
                                     translation.detach(), need=need, algo=ctx.algo)
        return (None, *_cast_grads(want, pb, (image, points, rotation, translation)))


def sample_smooth_ad(image, points, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample_smooth` (torch autograd) with respect to image, points, rotation and translation
    (tensors); the tangents are those of `sample_smooth_pullback_`."""
    return _SampleSmoothFn.apply(algo, image, points, rotation, translation)
