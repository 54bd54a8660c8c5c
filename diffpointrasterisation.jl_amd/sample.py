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

import ctypes
from collections import namedtuple

import torch

from . import _lib
from .interface import (_REFUSED, DimensionMismatch, _SUFFIX, _algo_name, _allocate, _canonicalise, _grid_arr,
                        _is_grid_layout, _ptr, _stream_ptr, empty_grid, to_grid_layout)

SamplePullbackResult = namedtuple("SamplePullbackResult", ["image", "points", "rotation", "translation"])
_NAMES = SamplePullbackResult._fields
_OPS = {"raster": _lib.OP_RASTER, "sample": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}


def resolve_algo_sample(op: str, grid_size, n_points: int, batch: int, n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a sampling call (dpr_resolve_algo_sample);
    op is "sample" (or "raster") for the forward and "pullback"."""
    g = _grid_arr(grid_size)
    rc = _lib.lib().dpr_resolve_algo_sample(_OPS[op], n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p),
                                            n_points, batch)
    return _algo_name(rc)


def workspace_bytes_sample(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                           algo: str = "auto") -> int:
    """dpr_workspace_bytes_sample_ex_*: device bytes a sampling call needs."""
    g = _grid_arr(grid_size)
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_sample_ex_{_SUFFIX[dtype]}")(
        _OPS[op], _lib.ALGOS[algo], 0, n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p), n_points, batch)
    if need == _REFUSED:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, _lib.last_error())
    return int(need)


def _workspace(op, algo_c, suf, n_in, grid, P, B, device, workspace):
    g = _grid_arr(grid)
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_sample_ex_{suf}")(
        op, algo_c, 0, n_in, len(grid), g.ctypes.data_as(ctypes.c_void_p), P, B)
    # (a refused query: the entry point itself reports the status, before any launch)
    return _allocate(0 if need == _REFUSED else need, device, workspace)


def _image(image, c):
    """The image in the grid layout of `empty_grid`, promoted dtype, checked against the poses."""
    dev, n_out = c["device"], c["n_out"]
    if not isinstance(image, torch.Tensor) or image.device != dev:
        raise RuntimeError("image must be a tensor on the same HIP device as points")
    expect_ndim = n_out + (0 if c["single"] else 1)
    if image.ndim != expect_ndim:
        raise DimensionMismatch(f"image has {image.ndim} dims, expected {expect_ndim} for N_out={n_out}")
    if not c["single"] and image.shape[-1] != c["B"]:
        raise DimensionMismatch(f"image batch dim {image.shape[-1]} != number of poses {c['B']}")
    img = image.to(c["dtype"])
    if not _is_grid_layout(img):
        img = to_grid_layout(img)
    return img


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
    img = _image(image, c)
    v = _values_view(values, c, "values")
    if values.dtype != c["dtype"]:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {c['dtype']}")
    if not v.is_contiguous():
        raise ValueError("values must have the point index fastest (a (P, B) transposed view of a (B, P) tensor)")
    n_in, n_out, P, B = c["n_in"], c["n_out"], c["P"], c["B"]
    grid = tuple(img.shape[:n_out])
    g = _grid_arr(grid)
    suf = _SUFFIX[c["dtype"]]
    algo_c = _lib.ALGOS[algo]
    with torch.cuda.device(c["device"]):
        ws, ws_bytes = _workspace(_lib.OP_RASTER, algo_c, suf, n_in, grid, P, B, c["device"], workspace)
        fn = getattr(_lib.lib(), f"dpr_sample_ex_{suf}")
        _lib.check(fn(_stream_ptr(c["device"]), algo_c, 0, n_in, n_out, g.ctypes.data_as(ctypes.c_void_p), P, B,
                      _ptr(v), _ptr(img), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]), _ptr(ws), ws_bytes))
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
    dev, dtype, P, B, n_in, n_out = c["device"], c["dtype"], c["P"], c["B"], c["n_in"], c["n_out"]
    img = _image(image, c)
    dv = _values_view(ds_dvalues, c, "ds_dvalues").to(dtype).contiguous()
    grid = tuple(img.shape[:n_out])
    g = _grid_arr(grid)

    def out_buf(buf, shape, name):
        if buf is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if (not isinstance(buf, torch.Tensor) or buf.device != dev or buf.dtype != dtype
                or tuple(buf.shape) != tuple(shape) or not buf.is_contiguous()):
            raise DimensionMismatch(f"{name}: need a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
        return buf

    d_img = d_pts = d_rot = d_trans = None
    if "image" in need:
        if ds_dimage is None:
            d_img = empty_grid(grid, None if c["single"] else B, dtype, dev)
        else:
            if (not isinstance(ds_dimage, torch.Tensor) or ds_dimage.device != dev or ds_dimage.dtype != dtype
                    or tuple(ds_dimage.shape) != tuple(image.shape) or not _is_grid_layout(ds_dimage)):
                raise DimensionMismatch(f"ds_dimage: need a {dtype} tensor of shape {tuple(image.shape)} on {dev} "
                                        "in the memory order of empty_grid")
            d_img = ds_dimage
    if "points" in need:
        d_pts = out_buf(ds_dpoints, (P, n_in), "ds_dpoints")
    if "rotation" in need:
        if ds_drotation is not None:
            rv = ds_drotation.transpose(-1, -2) if not c["single"] else ds_drotation.t()[None]
            if rv.shape != (B, n_in, n_out) or not rv.is_contiguous() or rv.dtype != dtype or rv.device != dev:
                raise DimensionMismatch(
                    "ds_drotation must be a (B, N_out, N_in) transposed view of a contiguous (B, N_in, N_out) buffer")
            d_rot = rv
        else:
            d_rot = torch.empty((B, n_in, n_out), dtype=dtype, device=dev)
    if "translation" in need:
        d_trans = out_buf(None if ds_dtranslation is None else ds_dtranslation.reshape(B, n_out), (B, n_out),
                          "ds_dtranslation")
    suf = _SUFFIX[dtype]
    algo_c = _lib.ALGOS[algo]
    with torch.cuda.device(dev):
        ws, ws_bytes = _workspace(_lib.OP_PULLBACK, algo_c, suf, n_in, grid, P, B, dev, workspace)
        fn = getattr(_lib.lib(), f"dpr_sample_pullback_ex_{suf}")
        _lib.check(fn(_stream_ptr(dev), algo_c, 0, n_in, n_out, g.ctypes.data_as(ctypes.c_void_p), P, B,
                      _ptr(dv), _ptr(img), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]), _ptr(d_img),
                      _ptr(d_pts), _ptr(d_rot), _ptr(d_trans), _ptr(ws), ws_bytes))
    rot_math = None if d_rot is None else d_rot.transpose(1, 2)
    if c["single"]:
        return SamplePullbackResult(d_img, d_pts, None if rot_math is None else rot_math[0],
                                    None if d_trans is None else d_trans[0])
    return SamplePullbackResult(d_img, d_pts, rot_math, d_trans)


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
        grads = [None]
        for name, t in zip(_NAMES, (image, points, rotation, translation)):
            gr = getattr(pb, name)
            grads.append(None if gr is None else gr.reshape(t.shape).to(t.dtype))
        return tuple(grads)


def sample_ad(image, points, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample` (torch autograd) with respect to image, points, rotation and translation
    (tensors); the tangents are those of `sample_pullback_`."""
    return _SampleFn.apply(algo, image, points, rotation, translation)
