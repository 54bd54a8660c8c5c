"""The argument and output plumbing every op family goes through (private).

  _canonicalise       the reference's dispatch funnel: defaults, single pose -> batch of one, dimension errors,
                      contiguous device buffers in the C ABI's layout
  _image              an image-shaped argument (out, ds_dout, target, image, out_dot) checked against the poses
  _out_buf, _rotation_buf, _per_pose
                      preallocated or new gradient outputs, and their single-pose unwrapping
  _launch             workspace query, allocation and the entry point call on torch's current stream
  _workspace_bytes, _resolve, _op_code
                      the bodies of the public workspace_bytes* / resolve_algo* queries
  _save, _restore, _cast_grads
                      the autograd rules' "tensor or constant" optional arguments and gradients

`DimensionMismatch`, `ColumnMajorRotation`, `column_major_rotation`, `empty_grid` and `to_grid_layout` are public
through `interface`, which re-exports them.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Optional, Sequence

import torch

from . import _lib

_SUFFIX = {torch.float32: "f32", torch.float64: "f64"}

# what a workspace query returns when it refuses the call (SIZE_MAX)
_REFUSED = ctypes.c_size_t(-1).value

_OPS = {"raster": _lib.OP_RASTER, "sample": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK,
        "residual_pullback": _lib.OP_RESIDUAL_PULLBACK}


class DimensionMismatch(ValueError):
    """Counterpart of Julia's DimensionMismatch thrown by the reference's @argcheck's."""


# --------------------------------------------------------------------------- layouts
def empty_grid(grid_size: Sequence[int], batch: Optional[int], dtype, device) -> torch.Tensor:
    """Allocate an `out`/`ds_dout`-shaped array with the reference's memory order
    (`similar(points, T, (grid_size..., B))`, src/interface.jl:67-74): returns a view
    of shape grid_size (+ (B,)) whose axis 1 is the fastest in memory."""
    shape = tuple(int(n) for n in grid_size) + (() if batch is None else (int(batch),))
    buf = torch.empty(tuple(reversed(shape)), dtype=dtype, device=device)
    return buf.permute(*reversed(range(len(shape))))


def to_grid_layout(t: torch.Tensor) -> torch.Tensor:
    """Copy an arbitrary-strided [i_1..i_N(,b)] tensor into the reference memory order."""
    out = empty_grid(t.shape, None, t.dtype, t.device)
    out.copy_(t)
    return out


def _is_grid_layout(t: torch.Tensor) -> bool:
    return t.permute(*reversed(range(t.ndim))).is_contiguous()


class ColumnMajorRotation:
    """A rotation argument already in the memory order of the C ABI (`Vector{SMatrix}`: every pose
    column-major), made once with `column_major_rotation` and accepted wherever a rotation tensor
    is.  For a torch tensor that order is a transpose + copy, two small kernels per call (2 x 4.4 us
    inside a 0.37 ms step); a caller whose pose does not change between calls -- or who keeps its
    pose in this order anyway, as a Julia host does -- skips them.  (Caching the copy per tensor and
    `_version` is not safe: writes through `.data`, as torch.autograd.gradcheck does, do not bump
    the version.)"""

    def __init__(self, cm: torch.Tensor, single: bool):
        self.cm, self.single = cm, single  # cm: contiguous (B, N_in, N_out)

    @property
    def ndim(self):
        return 2 if self.single else 3

    @property
    def shape(self):
        B, n_in, n_out = self.cm.shape
        return (n_out, n_in) if self.single else (B, n_out, n_in)

    @property
    def dtype(self):
        return self.cm.dtype


def column_major_rotation(rotation: torch.Tensor, dtype=None) -> ColumnMajorRotation:
    """(N_out, N_in) or (B, N_out, N_in) rotation tensor -> `ColumnMajorRotation` (a snapshot: later
    changes of `rotation` are not seen)."""
    r = rotation if dtype is None else rotation.to(dtype)
    single = r.ndim == 2
    if r.ndim not in (2, 3):
        raise DimensionMismatch("rotation must be (N_out, N_in) or (B, N_out, N_in)")
    r = r[None] if single else r
    return ColumnMajorRotation(r.transpose(1, 2).contiguous(), single)


# --------------------------------------------------------------------------- the funnel
def _promote(*tensors) -> torch.dtype:
    """promote_type over the array arguments (src/interface.jl:63-64).  Python scalars and
    lists are weakly typed and do not take part (they adopt the promoted dtype)."""
    dt = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            continue
        d = t.dtype
        if not d.is_floating_point:  # Bool / Int rotations such as I(2) (README.md:36)
            continue
        dt = d if dt is None else torch.promote_types(dt, d)
    if dt is None:
        dt = torch.get_default_dtype()
    if dt not in _SUFFIX:
        raise TypeError(f"libdpr supports float32/float64, got {dt}")
    return dt


def _device_of(points: torch.Tensor) -> torch.device:
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor on a HIP device")
    if points.device.type != "cuda":
        raise RuntimeError(
            "DiffPointRasterisation MI355X backend: `points` lives on "
            f"{points.device}; there is no CPU path in this package (device tensors required)."
        )
    return points.device


def _as(t, dtype, device, shape=None, name="argument") -> torch.Tensor:
    t = torch.as_tensor(t, dtype=dtype, device=device) if not isinstance(t, torch.Tensor) else t.to(
        device=device, dtype=dtype)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise DimensionMismatch(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _scalar(x) -> torch.Tensor:
    """Single-pose scalar argument -> 1-element vector (src/interface.jl:113-116) without
    rounding a Python float through float32."""
    if isinstance(x, torch.Tensor):
        return x.reshape(1)
    return torch.as_tensor(x, dtype=torch.float64).reshape(1)


def _check_dims(n_in_pts, rot_shape, trans_shape):
    """Step 5 of the reference funnel: explicit dimension errors
    (src/interface.jl:137-162, 315-366)."""
    n_out_rot, n_in_rot = rot_shape[-2], rot_shape[-1]
    n_out_trans = trans_shape[-1]
    if n_out_trans != n_out_rot:
        raise DimensionMismatch(
            f"Row dimension of rotation (got {n_out_rot}) and translation (got {n_out_trans}) must agree!")
    if n_in_rot != n_in_pts:
        raise DimensionMismatch(
            f"Column dimension of rotation (got {n_in_rot}) and points (got {n_in_pts}) must agree!")


def _canonicalise(points, rotation, translation, background, out_weight, point_weight, extra=()):
    """Steps 2-4 of the funnel: defaults (None == FillArrays Zeros/Ones -> NULL pointer),
    single pose -> batch of one, contiguous device buffers in the reference layout."""
    device = _device_of(points)
    if points.ndim != 2:
        raise DimensionMismatch(f"points must be (P, N_in), got {tuple(points.shape)}")
    pre = rotation if isinstance(rotation, ColumnMajorRotation) else None
    if pre is not None:
        rotation_t = pre.cm.transpose(1, 2)  # (a view in the mathematical shape, for the checks below)
        rotation_t = rotation_t[0] if pre.single else rotation_t
    else:
        rotation_t = rotation if isinstance(rotation, torch.Tensor) else torch.as_tensor(rotation)
    translation_t = translation if isinstance(translation, torch.Tensor) else torch.as_tensor(translation)
    single = rotation_t.ndim == 2  # src/interface.jl:67 `rotation isa AbstractMatrix`
    if rotation_t.ndim not in (2, 3):
        raise DimensionMismatch("rotation must be (N_out, N_in) or (B, N_out, N_in)")
    dtype = _promote(points, rotation_t, translation_t, background, out_weight, point_weight, *extra)
    if single:
        rotation_t = rotation_t[None]
        if translation_t.ndim != 1:
            raise DimensionMismatch("single-pose translation must be a vector")
        translation_t = translation_t[None]
        background = None if background is None else _scalar(background)
        out_weight = None if out_weight is None else _scalar(out_weight)
    if translation_t.ndim != 2:
        raise DimensionMismatch("batched translation must be (B, N_out)")
    P, n_in = points.shape
    _check_dims(n_in, rotation_t.shape, translation_t.shape)
    B, n_out = rotation_t.shape[0], rotation_t.shape[1]
    if translation_t.shape[0] != B:
        raise DimensionMismatch(
            f"batch sizes differ: rotation {B}, translation {translation_t.shape[0]}")
    pts = _as(points, dtype, device)
    # Vector{SMatrix}: each pose column-major == row-major of the transpose
    if pre is not None and pre.cm.dtype == dtype and pre.cm.device == device:
        rot_cm = pre.cm
    else:
        rot_cm = _as(rotation_t, dtype, device).transpose(1, 2).contiguous()
    trans = _as(translation_t, dtype, device)
    bg = None if background is None else _as(background, dtype, device, (B,), "background")
    ow = None if out_weight is None else _as(out_weight, dtype, device, (B,), "out_weight")
    if point_weight is not None and tuple(torch.as_tensor(point_weight).shape) != (P,):
        raise DimensionMismatch(  # @argcheck length(point_weight) == n_points, src/raster.jl:23
            f"length(point_weight) = {tuple(torch.as_tensor(point_weight).shape)} != n_points = {P}")
    pw = None if point_weight is None else _as(point_weight, dtype, device, (P,), "point_weight")
    return dict(device=device, dtype=dtype, single=single, P=P, B=B, n_in=n_in, n_out=n_out,
                points=pts, rot=rot_cm, trans=trans, bg=bg, ow=ow, pw=pw)


def _alloc_like(points, rotation, translation, *optional):
    """(device, dtype, batch) of an allocating forward's result, from the arguments before they are
    canonicalised; batch is None for a single pose."""
    device = _device_of(points)
    rot_like = isinstance(rotation, (torch.Tensor, ColumnMajorRotation))
    rot_nd = rotation.ndim if rot_like else torch.as_tensor(rotation).ndim
    dtype = _promote(points, rotation.cm if isinstance(rotation, ColumnMajorRotation) else rotation,
                     translation, *optional)
    batch = None if rot_nd == 2 else (rotation.shape[0] if rot_like else len(rotation))
    return device, dtype, batch


def _image(t, name, c, axes=(), *, out=False, grid=None):
    """An image-shaped argument of the canonical call `c`: grid + `axes` ((name, size) pairs: channels,
    tangents) + (B,) for a batch.  `out=True`: an output, which must already have the promoted dtype and the
    memory order of `empty_grid`.  Otherwise an input, returned in that dtype and order (a copy where it
    differs).  `grid`: the grid size it must have (that of another image)."""
    if not isinstance(t, torch.Tensor) or t.device != c["device"]:
        raise RuntimeError(f"{name} must be a tensor on the same HIP device as points")
    n_out = c["n_out"]
    axes = tuple(axes) + (() if c["single"] else (("poses", c["B"]),))
    tail = tuple(n for _, n in axes)
    if t.ndim != n_out + len(tail):  # @argcheck N_out == N_out_p1 - 1, src/raster.jl:14
        raise DimensionMismatch(f"{name} has {t.ndim} dims, expected {n_out + len(tail)} for N_out={n_out}")
    if tuple(t.shape[n_out:]) != tail:  # src/raster.jl:17-21
        raise DimensionMismatch(f"{name} trailing dims {tuple(t.shape[n_out:])} must be {tail} "
                                f"({', '.join(a for a, _ in axes)})")
    if grid is not None and tuple(t.shape[:n_out]) != tuple(grid):
        raise DimensionMismatch(f"{name} grid {tuple(t.shape[:n_out])} != {tuple(grid)}")
    if out:
        if t.dtype != c["dtype"]:
            raise TypeError(f"{name} dtype {t.dtype} != promoted argument dtype {c['dtype']}")
        if not _is_grid_layout(t):
            raise ValueError(f"{name} must have the memory order of empty_grid (use empty_grid / to_grid_layout)")
        return t
    t = t.to(c["dtype"])
    return t if _is_grid_layout(t) else to_grid_layout(t)


# --------------------------------------------------------------------------- gradient outputs
def _out_buf(given, shape, name, c, *, reshape=False, grid_layout=False):
    """A gradient output of `shape`: the caller's buffer `given` (reshaped first with reshape=True), which
    must be contiguous -- or with grid_layout=True in the memory order of `empty_grid` -- with the promoted
    dtype on the device; or a new one."""
    dtype, dev = c["dtype"], c["device"]
    if given is None:
        return empty_grid(shape, None, dtype, dev) if grid_layout else torch.empty(shape, dtype=dtype, device=dev)
    if reshape:
        given = given.reshape(shape)
    if (not isinstance(given, torch.Tensor) or given.device != dev or given.dtype != dtype
            or tuple(given.shape) != tuple(shape)
            or not (_is_grid_layout(given) if grid_layout else given.is_contiguous())):
        order = "in the memory order of empty_grid" if grid_layout else "contiguous"
        raise DimensionMismatch(f"{name}: need a {dtype} tensor of shape {tuple(shape)} on {dev}, {order}")
    return given


def _rotation_buf(given, c):
    """The ds_drotation output: the caller's (B, N_out, N_in) (single pose: (N_out, N_in)) transposed view of
    a contiguous (B, N_in, N_out) buffer -- the column-major (N_out, N_in, B) of the C ABI -- or a new one."""
    B, n_in, n_out = c["B"], c["n_in"], c["n_out"]
    if given is None:
        return torch.empty((B, n_in, n_out), dtype=c["dtype"], device=c["device"])
    rv = given.t()[None] if c["single"] else given.transpose(-1, -2)
    if (rv.shape != (B, n_in, n_out) or not rv.is_contiguous() or rv.dtype != c["dtype"]
            or rv.device != c["device"]):
        raise DimensionMismatch(
            f"ds_drotation must be a (B, N_out, N_in) transposed view of a contiguous (B, N_in, N_out) "
            f"{c['dtype']} buffer on {c['device']} (column-major N_out x N_in per pose)")
    return rv


def _per_pose(c, d_rot, *per_pose):
    """The rotation gradient in the mathematical (B, N_out, N_in) shape (a view of its column-major buffer),
    then `per_pose`; for a single pose, pose 0 of each.  None stays None."""
    rot = None if d_rot is None else d_rot.transpose(1, 2)
    if not c["single"]:
        return (rot,) + per_pose
    return tuple(None if t is None else t[0] for t in (rot,) + per_pose)


# --------------------------------------------------------------------------- libdpr calls
def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_ptr(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _grid_arr(grid):
    """The grid sizes as the int64 array the C ABI reads."""
    import numpy as np

    return np.asarray(tuple(int(n) for n in grid), dtype=np.int64)


def _grid_call(fn, head, n_in, grid, P, B, *rest):
    """fn(*head, n_in, n_out, grid, P, B, *rest): the argument order every query and entry point shares.
    The grid array lives until fn returns."""
    g = _grid_arr(grid)
    return fn(*head, n_in, len(g), g.ctypes.data_as(ctypes.c_void_p), P, B, *rest)


def _algo_name(rc: int) -> str:
    """Name of a resolved DPR_ALGO_* value; an error status raises."""
    if rc < 0:
        _lib.check(rc)
    return {v: k for k, v in _lib.ALGOS.items()}[rc]


def _op_code(op: str, accepted) -> int:
    """DPR_OP_* of `op`, one of the family's `accepted` names (KeyError otherwise)."""
    code = _OPS[op]
    if op not in accepted:
        raise KeyError(op)
    return code


def _resolve(name: str, head, grid_size, n_points, batch, n_in, *tail) -> str:
    """Body of the public resolve_algo*: libdpr's `name` query, answered as an algorithm name."""
    return _algo_name(_grid_call(getattr(_lib.lib(), name), head, n_in, grid_size, n_points, batch, *tail))


def _workspace_bytes(family: str, head, dtype, grid_size, n_points, batch, n_in, *tail) -> int:
    """Body of the public workspace_bytes*: dpr_workspace_bytes{family}_ex_* (a refused query raises)."""
    fn = getattr(_lib.lib(), f"dpr_workspace_bytes{family}_ex_{_SUFFIX[dtype]}")
    need = _grid_call(fn, head, n_in, grid_size, n_points, batch, *tail)
    if need == _REFUSED:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, _lib.last_error())
    return int(need)


def _allocate(need, device, workspace):
    """(workspace, bytes) for a queried `need`: none for 0, else the caller's buffer if it holds `need` bytes on
    `device`, or a new one."""
    if need == 0:
        return None, 0
    if workspace is not None:
        if workspace.device != device or workspace.numel() * workspace.element_size() < need:
            raise ValueError(f"workspace too small: need {need} bytes")
        return workspace, workspace.numel() * workspace.element_size()
    return torch.empty(need, dtype=torch.uint8, device=device), need


def _launch(family, entry, op, c, grid, algo, flags, workspace, *args, tail=(), refused_raises=False,
            workspace_required=None):
    """One call of a libdpr entry point for the canonical call `c`, enqueued on torch's current stream:

        need = dpr_workspace_bytes{family}_ex_*([op,] algo, flags, n_in, n_out, grid, P, B, *tail)
        {entry}_*(stream, algo, flags, n_in, n_out, grid, P, B, *tail, *args, workspace, bytes)

    with tensors in `args` passed as device pointers (None: NULL).  The workspace is `workspace` if it holds
    `need` bytes, else a new one.  A refused query raises DprError with refused_raises=True; otherwise the
    entry point reports its own status, before any launch.  `workspace_required`: the ValueError raised after
    the query when the caller passed no workspace."""
    suf = _SUFFIX[c["dtype"]]
    algo_c = _lib.ALGOS[algo]
    L = _lib.lib()
    with torch.cuda.device(c["device"]):
        head = (algo_c, flags) if op is None else (op, algo_c, flags)
        need = _grid_call(getattr(L, f"dpr_workspace_bytes{family}_ex_{suf}"), head, c["n_in"], grid, c["P"],
                          c["B"], *tail)
        if need == _REFUSED:
            if refused_raises:
                raise _lib.DprError(_lib.ERR_INVALID_ARG, _lib.last_error())
            need = 0
        ws, ws_bytes = _allocate(need, c["device"], workspace)
        if workspace_required is not None and workspace is None:
            raise ValueError(workspace_required)
        ptrs = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        _lib.check(_grid_call(getattr(L, f"{entry}_{suf}"), (_stream_ptr(c["device"]), algo_c, flags),
                              c["n_in"], grid, c["P"], c["B"], *tail, *ptrs, _ptr(ws), ws_bytes))


# --------------------------------------------------------------------------- autograd
def _detach(t):
    return t.detach() if isinstance(t, torch.Tensor) else t


def _save(ctx, tensors, optional):
    """save_for_backward(*tensors, *the tensors among `optional`); the other optional arguments are
    constants kept on ctx.  Returns what was saved."""
    ctx.opt_is_tensor = tuple(isinstance(t, torch.Tensor) for t in optional)
    ctx.opt = tuple(None if isinstance(t, torch.Tensor) else t for t in optional)
    saved = (*tensors, *[t for t in optional if isinstance(t, torch.Tensor)])
    ctx.save_for_backward(*saved)
    return saved


def _restore(ctx, n):
    """(the first n saved tensors, the optional arguments) of `_save`."""
    saved = ctx.saved_tensors
    rest = iter(saved[n:])
    return saved[:n], [next(rest) if is_t else k for is_t, k in zip(ctx.opt_is_tensor, ctx.opt)]


_Like = namedtuple("_Like", ["shape", "dtype"])


def _cast_grads(need, grads, like):
    """Autograd's gradients: grads[k] reshaped and cast to the shape and dtype of like[k] (an input, or a
    `_Like`), None where need[k] is false."""
    return tuple(g.reshape(t.shape).to(t.dtype) if n else None for n, g, t in zip(need, grads, like))
