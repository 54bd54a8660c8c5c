"""Smooth sampling at the points of rigid bodies: `sample_smooth` through one pose per (image, body), forward and
pullback (dpr_sample_smooth_bodies_ex_* / dpr_sample_smooth_bodies_pullback_ex_*, include/dpr.h "SMOOTH SAMPLING,
RIGID BODIES").

    values[p, b] = sum_s in-grid image[j0 + s, b] * prod_d w_d(s_d),   s in {-1, 0, +1}^N_out

with the cell and the weights of `raster_smooth` under pose (b, body[p]); 0 for a point rejected in image b or whose
body lies outside [0, K).  The transpose of `raster_smooth_bodies` with respect to the point weights, with one weight
per (point, image): score a map at the atoms of K domains, each under its own pose, and get the exact gradient of
that score in all B * K poses and in the points.  One call in the place of K subset calls of `sample_smooth`.

Shapes: image / ds_dimage grid_size (one image) or grid_size + (B,) in the memory order of `empty_grid`; points
(P, N_in); body (P,) int32 or int64, no gradient; rotation (B, K, N_out, N_in) and translation (B, K, N_out), or
without the B axis for one image; values / ds_dvalues (P, B) with the point index fastest, (P,) for one image.
Sort the cloud by body.  (N_in, N_out): (2,2), (3,3), (3,2).

Algorithms: "atomic" (forward and pullback), "tiled" (pullback: ds_dimage through the binning of the tiled
`raster_smooth_bodies`, the images in groups; `max_pose_group` bounds a group and is refused by every other path),
"auto".  There is no public workspace query for this family: every call asks
dpr_workspace_bytes_sample_smooth_bodies_ex_* itself and allocates, or checks the `workspace` the caller passed (a
uint8 tensor on the device); the C query is reachable through `lib()`.
"""
from __future__ import annotations

import torch

from . import _lib
from ._args import _cast_grads, _image, _launch, _op_code, _out_buf, _resolve
from .bodies import _canonicalise_bodies, _check_shapes, _rotation_buf
from .sample import SamplePullbackResult, _values_view

_NAMES = SamplePullbackResult._fields
_ACCEPTED_OPS = ("raster", "sample", "pullback")


def resolve_algo_sample_smooth_bodies(op: str, grid_size, n_points: int, batch: int, n_bodies: int,
                                      n_in: int) -> str:
    """Name of the algorithm `algo="auto"` picks for a call (dpr_resolve_algo_sample_smooth_bodies); op is "sample"
    (or "raster") for the forward and "pullback"."""
    return _resolve("dpr_resolve_algo_sample_smooth_bodies", (_op_code(op, _ACCEPTED_OPS),), grid_size, n_points,
                    batch, n_in, n_bodies)


def sample_smooth_bodies(image, points, body, rotation, translation, *, algo: str = "auto",
                         workspace=None) -> torch.Tensor:
    """Allocating forward: values (P,) for one image (rotation is (K, N_out, N_in)), (P, B) with the point index
    fastest for a batch."""
    c = _canonicalise_bodies(points, body, rotation, translation, None, None, None, extra=(image,))
    P, B = c["P"], c["B"]
    if c["single"]:
        values = torch.empty((P,), dtype=c["dtype"], device=c["device"])
    else:
        values = torch.empty((B, P), dtype=c["dtype"], device=c["device"]).t()
    return sample_smooth_bodies_(values, image, points, body, rotation, translation, algo=algo, workspace=workspace)


def sample_smooth_bodies_(values, image, points, body, rotation, translation, *, algo: str = "auto",
                          workspace=None) -> torch.Tensor:
    """In-place forward: `values` ((P,) or (P, B), point index fastest) is overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_bodies(points, body, rotation, translation, None, None, None, extra=(image,))
    img = _image(image, "image", c)
    v = _values_view(values, c, "values")
    if values.dtype != c["dtype"]:
        raise TypeError(f"values dtype {values.dtype} != promoted argument dtype {c['dtype']}")
    if not v.is_contiguous():
        raise ValueError("values must have the point index fastest (a (P, B) transposed view of a (B, P) tensor)")
    _launch("_sample_smooth_bodies", "dpr_sample_smooth_bodies_ex", _lib.OP_RASTER, c, img.shape[: c["n_out"]], algo,
            0, workspace, v, img, c["points"], c["body"], c["rot"], c["trans"], tail=(c["K"],))
    return values


def sample_smooth_bodies_pullback_(ds_dvalues, image, points, body, rotation, translation, *, ds_dimage=None,
                                   ds_dpoints=None, ds_drotation=None, ds_dtranslation=None, need=_NAMES,
                                   algo: str = "auto", workspace=None, max_pose_group: int = 0,
                                   grid_size=None) -> SamplePullbackResult:
    """Pullback of `sample_smooth_bodies`.  `need` names the gradients wanted (any of "image", "points", "rotation",
    "translation"); the others are neither computed nor written and come back as None.  Keyword outputs are
    pre-allocated buffers, OVERWRITTEN and returned by identity: ds_dimage shaped like image, ds_dpoints (P, N_in),
    ds_drotation shaped like rotation (a transposed view of a contiguous (B, K, N_in, N_out) buffer), ds_dtranslation
    like translation.  `image` may be None when only "image" is needed (ds_dimage does not depend on it); the grid
    then comes from the ds_dimage buffer or from `grid_size`.  `max_pose_group` (1..16, 0 = default): the most images
    "tiled" bins together (DPR_FLAG_MAX_POSE_GROUP)."""
    _check_shapes(points, body, rotation, translation)
    flags = _lib.flag_max_pose_group(max_pose_group)  # (a value outside 0..16 raises before anything else)
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
    c = _canonicalise_bodies(points, body, rotation, translation, None, None, None, extra=(image, ds_dvalues))
    P, B, K, n_in, n_out, single = c["P"], c["B"], c["K"], c["n_in"], c["n_out"], c["single"]
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
        d_img = _out_buf(ds_dimage, grid + (() if single else (B,)), "ds_dimage", c, grid_layout=True)
    if "points" in need:
        d_pts = _out_buf(ds_dpoints, (P, n_in), "ds_dpoints", c)
    if "rotation" in need:
        d_rot = _rotation_buf(ds_drotation, c)
    if "translation" in need:
        d_trans = _out_buf(ds_dtranslation, (B, K, n_out), "ds_dtranslation", c, reshape=single)
    _launch("_sample_smooth_bodies", "dpr_sample_smooth_bodies_pullback_ex", _lib.OP_PULLBACK, c, grid, algo, flags,
            workspace, dv, img, c["points"], c["body"], c["rot"], c["trans"], d_img, d_pts, d_rot, d_trans,
            tail=(K,))
    rot = None if d_rot is None else d_rot.transpose(-1, -2)
    if single:
        rot = None if rot is None else rot[0]
        d_trans = None if d_trans is None else d_trans[0]
    return SamplePullbackResult(d_img, d_pts, rot, d_trans)


class _SampleSmoothBodiesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, algo, body, image, points, rotation, translation):
        values = sample_smooth_bodies(image.detach(), points.detach(), body, rotation.detach(), translation.detach(),
                                      algo="atomic" if algo == "tiled" else algo)  # (the forward has no tiled variant)
        ctx.save_for_backward(image, points, rotation, translation, body)
        ctx.algo = algo
        return values

    @staticmethod
    def backward(ctx, ds_dvalues):
        image, points, rotation, translation, body = ctx.saved_tensors
        want = ctx.needs_input_grad[2:]  # (image, points, rotation, translation)
        need = tuple(n for n, w in zip(_NAMES, want) if w)
        if not need:
            return None, None, None, None, None, None
        pb = sample_smooth_bodies_pullback_(ds_dvalues.detach(), image.detach(), points.detach(), body,
                                            rotation.detach(), translation.detach(), need=need, algo=ctx.algo)
        return (None, None, *_cast_grads(want, pb, (image, points, rotation, translation)))


def sample_smooth_bodies_ad(image, points, body, rotation, translation, *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `sample_smooth_bodies` (torch autograd) with respect to image, points, rotation and
    translation (tensors); `body` has no gradient.  The tangents are those of `sample_smooth_bodies_pullback_`."""
    _check_shapes(points, body, rotation, translation)
    return _SampleSmoothBodiesFn.apply(algo, body, image, points, rotation, translation)
