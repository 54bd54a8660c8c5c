"""Per-pose point clouds: a different cloud for every pose, forward and pullback
(dpr_raster_clouds_ex_* / dpr_raster_pullback_clouds_ex_*, include/dpr.h "PER-POSE CLOUDS").

For pose b, with its own cloud points[b]:

    out[i.., b] = background[b] + out_weight[b] * sum_p point_weight[b, p] * voxel_weight(i..; R_b points[b, p] + t_b)

Plane b is exactly `raster(grid, points[b], R_b, t_b, background[b], out_weight[b], point_weight[b])`, and the
pullback decomposes the same way (ds_dpoints[b] is the single-pose gradient of pose b: no sum over poses).  Shapes:

  points, ds_dpoints       (B, P, N_in) contiguous
  point_weight             (B, P), or (P,) shared by all poses; its gradient has the argument's shape ((P,): the
                           sum over the poses; (B, P) when point_weight is None)
  rotation, translation,   batched as in `raster`: (B, N_out, N_in), (B, N_out), (B,), (B,)
  background, out_weight
  out, ds_dout             grid_size + (B,) in the memory order of `empty_grid`

Clouds of different sizes: pad them to a common P with point_weight 0 (a zero-weight point deposits nothing and
gets ds_dpoints 0).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .interface import (_REFUSED, ColumnMajorRotation, DimensionMismatch, PullbackResult, _SUFFIX, _algo_name,
                        _allocate, _as, _canonicalise, _device_of, _grid_arr, _is_grid_layout, _promote, _ptr,
                        _stream_ptr, empty_grid, to_grid_layout)

_OPS = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}


def resolve_algo_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32) -> str:
    """Name of the algorithm `algo="auto"` picks for a per-pose cloud call (dpr_resolve_algo_clouds); op is
    "raster" or "pullback"; n_points is P, the points of each cloud.  The C query answers for fp32 data; an fp64
    pullback takes "atomic" where it answers "chunked" (include/dpr.h, PER-POSE CLOUDS)."""
    g = _grid_arr(grid_size)
    rc = _lib.lib().dpr_resolve_algo_clouds(_OPS[op], n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p),
                                            n_points, batch)
    name = _algo_name(rc)
    return "atomic" if (op == "pullback" and dtype == torch.float64 and name == "chunked") else name


def workspace_bytes_clouds(op: str, grid_size, n_points: int, batch: int, n_in: int, dtype=torch.float32,
                           algo: str = "auto") -> int:
    """dpr_workspace_bytes_clouds_ex_*: device bytes a per-pose cloud call needs."""
    g = _grid_arr(grid_size)
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_clouds_ex_{_SUFFIX[dtype]}")(
        _OPS[op], _lib.ALGOS[algo], 0, n_in, len(grid_size), g.ctypes.data_as(ctypes.c_void_p), n_points, batch)
    if need == _REFUSED:
        raise _lib.DprError(_lib.ERR_INVALID_ARG, _lib.last_error())
    return int(need)


def _workspace(op, algo_c, suf, n_in, grid, P, B, device, workspace, flags=0):
    g = _grid_arr(grid)
    need = getattr(_lib.lib(), f"dpr_workspace_bytes_clouds_ex_{suf}")(
        op, algo_c, flags, n_in, len(grid), g.ctypes.data_as(ctypes.c_void_p), P, B)
    # (a refused query: the entry point itself reports the status, before any launch)
    return _allocate(0 if need == _REFUSED else need, device, workspace)


def _shape(t):
    return tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(torch.as_tensor(t).shape)


def _check_shapes(points, rotation, translation, point_weight):
    """The shape errors of a per-pose cloud call, raised before anything else looks at the arguments."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("points must be a torch.Tensor on a HIP device")
    if points.ndim != 3:
        raise DimensionMismatch(f"points must be (B, P, N_in), got {tuple(points.shape)}")
    B, P, n_in = points.shape
    rs = tuple(rotation.shape) if isinstance(rotation, (torch.Tensor, ColumnMajorRotation)) else _shape(rotation)
    if len(rs) != 3:
        raise DimensionMismatch(f"per-pose clouds need batched poses: rotation (B, N_out, N_in), got {rs}")
    if rs[0] != B:
        raise DimensionMismatch(f"points hold {B} clouds, but rotation has {rs[0]} poses")
    if rs[2] != n_in:
        raise DimensionMismatch(f"Column dimension of rotation (got {rs[2]}) and points (got {n_in}) must agree!")
    ts = _shape(translation)
    if ts != (B, rs[1]):
        raise DimensionMismatch(f"translation must be (B, N_out) = {(B, rs[1])}, got {ts}")
    if point_weight is not None and _shape(point_weight) not in ((B, P), (P,)):
        raise DimensionMismatch(
            f"size(point_weight) = {_shape(point_weight)} must be (B, P) = {(B, P)} or (P,) = {(P,)}")


def _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight, extra=()):
    """_canonicalise of interface.py for (B, P, N_in) clouds: the pose arguments must be batched; point_weight
    (B, P) or (P,) becomes a contiguous (B, P) buffer.  Adds "shared_pw" (the argument was (P,))."""
    _check_shapes(points, rotation, translation, point_weight)
    device = _device_of(points)
    Bp, P, n_in = points.shape
    first = points[0] if Bp > 0 else points.new_empty((P, n_in))
    c = _canonicalise(first, rotation, translation, background, out_weight, None,
                      extra=(points, point_weight) + tuple(extra))
    B, dtype = c["B"], c["dtype"]
    if Bp != B:
        raise DimensionMismatch(f"points hold {Bp} clouds, but there are {B} poses")
    c["points"] = _as(points, dtype, device)
    c["shared_pw"] = False
    if point_weight is not None:
        shape = _shape(point_weight)
        if shape == (P,):
            c["shared_pw"] = True
            pw = _as(point_weight, dtype, device, (P,), "point_weight")
            c["pw"] = pw.unsqueeze(0).expand(B, P).contiguous()
        elif shape == (B, P):
            c["pw"] = _as(point_weight, dtype, device, (B, P), "point_weight")
        else:
            raise DimensionMismatch(f"size(point_weight) = {shape} must be (B, P) = {(B, P)} or (P,) = {(P,)}")
    return c


def raster_clouds(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                  *, algo: str = "auto", workspace=None) -> torch.Tensor:
    """Allocating forward: returns out[i_1..i_N, b] (the layout of `empty_grid(grid_size, B)`)."""
    _check_shapes(points, rotation, translation, point_weight)
    device = _device_of(points)
    dtype = _promote(points, rotation.cm if isinstance(rotation, ColumnMajorRotation) else rotation, translation,
                     background, out_weight, point_weight)
    out = empty_grid(tuple(grid_size), points.shape[0], dtype, device)
    return raster_clouds_(out, points, rotation, translation, background, out_weight, point_weight, algo=algo,
                          workspace=workspace)


def raster_clouds_(out, points, rotation, translation, background=None, out_weight=None, point_weight=None, *,
                   algo: str = "auto", workspace=None) -> torch.Tensor:
    """In-place forward: `out` (grid_size + (B,), memory order of `empty_grid`) is fully overwritten and returned.
    Enqueued on torch's current stream; not synchronised."""
    c = _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight)
    if not isinstance(out, torch.Tensor) or out.device != c["device"]:
        raise RuntimeError("out must be a tensor on the same HIP device as points")
    if out.ndim != c["n_out"] + 1:
        raise DimensionMismatch(f"out has {out.ndim} dims, expected {c['n_out'] + 1} for N_out={c['n_out']}")
    if out.shape[-1] != c["B"]:
        raise DimensionMismatch(f"out batch dim {out.shape[-1]} != number of poses {c['B']}")
    if out.dtype != c["dtype"]:
        raise TypeError(f"out dtype {out.dtype} != promoted argument dtype {c['dtype']}")
    if not _is_grid_layout(out):
        raise ValueError("out must have the reference memory order (use empty_grid/to_grid_layout)")
    grid = tuple(out.shape[: c["n_out"]])
    g = _grid_arr(grid)
    suf = _SUFFIX[c["dtype"]]
    algo_c = _lib.ALGOS[algo]
    with torch.cuda.device(c["device"]):
        ws, ws_bytes = _workspace(_lib.OP_RASTER, algo_c, suf, c["n_in"], grid, c["P"], c["B"], c["device"],
                                  workspace)
        fn = getattr(_lib.lib(), f"dpr_raster_clouds_ex_{suf}")
        _lib.check(fn(_stream_ptr(c["device"]), algo_c, 0, c["n_in"], c["n_out"], g.ctypes.data_as(ctypes.c_void_p),
                      c["P"], c["B"], _ptr(out), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]), _ptr(c["bg"]),
                      _ptr(c["ow"]), _ptr(c["pw"]), _ptr(ws), ws_bytes))
    return out


def raster_pullback_clouds_(ds_dout, points, rotation, translation, background=None, out_weight=None,
                            point_weight=None, *, ds_dpoints=None, ds_drotation=None, ds_dtranslation=None,
                            ds_dbackground=None, ds_dout_weight=None, ds_dpoint_weight=None, algo: str = "auto",
                            workspace=None, point_weight_grad: bool = True) -> PullbackResult:
    """Pullback of `raster_clouds`.  Keyword outputs are pre-allocated buffers, OVERWRITTEN and returned by
    identity: ds_dpoints (B, P, N_in); ds_drotation (B, N_out, N_in) as a transposed view of a contiguous
    (B, N_in, N_out) buffer; ds_dtranslation (B, N_out); ds_dbackground, ds_dout_weight (B,); ds_dpoint_weight
    shaped like point_weight ((P,): the sum over the poses; (B, P) when point_weight is None).
    `point_weight_grad=False` (DPR_FLAG_NO_POINT_WEIGHT_GRAD): ds_dpoint_weight is neither computed nor written
    and comes back as None."""
    c = _canonicalise_clouds(points, rotation, translation, background, out_weight, point_weight, extra=(ds_dout,))
    dev, dtype, P, B, n_in, n_out = c["device"], c["dtype"], c["P"], c["B"], c["n_in"], c["n_out"]
    if not isinstance(ds_dout, torch.Tensor) or ds_dout.device != dev:
        raise RuntimeError("ds_dout must be a tensor on the same HIP device as points")
    if ds_dout.ndim != n_out + 1:
        raise DimensionMismatch(f"ds_dout has {ds_dout.ndim} dims, expected {n_out + 1}")
    if ds_dout.shape[-1] != B:
        raise DimensionMismatch(f"ds_dout batch dim {ds_dout.shape[-1]} != number of poses {B}")
    gr = ds_dout.to(dtype)
    if not _is_grid_layout(gr):
        gr = to_grid_layout(gr)
    grid = tuple(gr.shape[:n_out])
    g = _grid_arr(grid)

    def out_buf(given, shape, name):
        if given is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if (not isinstance(given, torch.Tensor) or given.device != dev or given.dtype != dtype
                or tuple(given.shape) != tuple(shape) or not given.is_contiguous()):
            raise DimensionMismatch(f"{name}: need a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
        return given

    d_pts = out_buf(ds_dpoints, (B, P, n_in), "ds_dpoints")
    if ds_drotation is not None:
        rv = ds_drotation.transpose(-1, -2)
        if rv.shape != (B, n_in, n_out) or not rv.is_contiguous() or rv.dtype != dtype or rv.device != dev:
            raise DimensionMismatch(
                "ds_drotation must be a (B, N_out, N_in) transposed view of a contiguous (B, N_in, N_out) buffer")
        d_rot = rv
    else:
        d_rot = torch.empty((B, n_in, n_out), dtype=dtype, device=dev)
    d_trans = out_buf(ds_dtranslation, (B, n_out), "ds_dtranslation")
    d_bg = out_buf(ds_dbackground, (B,), "ds_dbackground")
    d_ow = out_buf(ds_dout_weight, (B,), "ds_dout_weight")
    if not point_weight_grad and ds_dpoint_weight is not None:
        raise ValueError("point_weight_grad=False and a ds_dpoint_weight buffer contradict each other")
    d_pw = d_pw_user = None
    if point_weight_grad:
        if c["shared_pw"]:
            d_pw_user = out_buf(ds_dpoint_weight, (P,), "ds_dpoint_weight")
            d_pw = torch.empty((B, P), dtype=dtype, device=dev)
        else:
            d_pw = d_pw_user = out_buf(ds_dpoint_weight, (B, P), "ds_dpoint_weight")
    suf = _SUFFIX[dtype]
    algo_c = _lib.ALGOS[algo]
    flags = 0 if point_weight_grad else _lib.FLAG_NO_POINT_WEIGHT_GRAD
    with torch.cuda.device(dev):
        ws, ws_bytes = _workspace(_lib.OP_PULLBACK, algo_c, suf, n_in, grid, P, B, dev, workspace, flags)
        fn = getattr(_lib.lib(), f"dpr_raster_pullback_clouds_ex_{suf}")
        _lib.check(fn(_stream_ptr(dev), algo_c, flags, n_in, n_out, g.ctypes.data_as(ctypes.c_void_p), P, B,
                      _ptr(gr), _ptr(c["points"]), _ptr(c["rot"]), _ptr(c["trans"]), _ptr(c["ow"]), _ptr(c["pw"]),
                      _ptr(d_pts), _ptr(d_rot), _ptr(d_trans), _ptr(d_bg), _ptr(d_ow), _ptr(d_pw), _ptr(ws),
                      ws_bytes))
        if c["shared_pw"] and d_pw is not None:
            torch.sum(d_pw, dim=0, out=d_pw_user)  # a weight shared by all poses: the sum of its per-pose gradients
    return PullbackResult(d_pts, d_rot.transpose(1, 2), d_trans, d_bg, d_ow, d_pw_user)


class _RasterCloudsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_size, algo, points, rotation, translation, background, out_weight, point_weight):
        det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
        out = raster_clouds(grid_size, det(points), det(rotation), det(translation), det(background),
                            det(out_weight), det(point_weight), algo=algo)
        ctx.opt_is_tensor = tuple(isinstance(t, torch.Tensor) for t in (background, out_weight, point_weight))
        ctx.opt = tuple(None if isinstance(t, torch.Tensor) else t for t in (background, out_weight, point_weight))
        ctx.save_for_backward(points, rotation, translation,
                              *[t for t in (background, out_weight, point_weight) if isinstance(t, torch.Tensor)])
        ctx.algo = algo
        return out

    @staticmethod
    def backward(ctx, ds_dout):
        saved = list(ctx.saved_tensors)
        points, rotation, translation = saved[:3]
        rest = saved[3:]
        opt = [rest.pop(0) if ctx.opt_is_tensor[k] else ctx.opt[k] for k in range(3)]
        det = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
        need = ctx.needs_input_grad  # (grid_size, algo, points, rotation, translation, bg, ow, pw)
        pb = raster_pullback_clouds_(ds_dout.detach(), det(points), det(rotation), det(translation), *map(det, opt),
                                     algo=ctx.algo, point_weight_grad=bool(ctx.opt_is_tensor[2] and need[7]))
        grads = [None, None,
                 pb.points.to(points.dtype) if need[2] else None,
                 pb.rotation.to(rotation.dtype) if need[3] else None,
                 pb.translation.to(translation.dtype) if need[4] else None]
        for k, gr in enumerate((pb.background, pb.out_weight, pb.point_weight)):
            t = opt[k]
            grads.append(gr.reshape(t.shape).to(t.dtype) if ctx.opt_is_tensor[k] and need[5 + k] else None)
        return tuple(grads)


def raster_clouds_ad(grid_size, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                     *, algo: str = "auto") -> torch.Tensor:
    """Differentiable `raster_clouds` (torch autograd) in points, rotation, translation, background, out_weight and
    point_weight (whichever are tensors that require grad); the tangents are those of `raster_pullback_clouds_`."""
    return _RasterCloudsFn.apply(tuple(grid_size), algo, points, rotation, translation, background, out_weight,
                                 point_weight)
