"""Smooth sampling at per-pose clouds held to the workspace and stream contract of include/dpr.h, in
the pattern of tests/test_sample_smooth_bodies_contract_gpu.py.

THE WORKSPACE CONTRACT: "The initial contents of the workspace do not matter: every piece of a layout is written by the
call before the call reads it.  The library writes only inside [workspace, workspace + workspace_bytes)."  The TILED
pullback runs on the interior view buf[4096 : 4096 + need] of a uint8 buffer whose two guard bands of 4096 bytes hold
0xA5, with `need` from dpr_workspace_bytes_sample_smooth_clouds_ex_* for the flags of the call, on three workspace
contents: zeros; stale (what a call with other clouds and poses left behind); every byte 0xFF (the all-ones key, the
largest index and count).  Afterwards the guards are unchanged and the four outputs, pre-filled with NaN, are finite
and match the reference -- for groups of one pose, of two (2 + 2 + 1) and the default (all five).  A workspace one byte
short is refused before any launch.

THE OUTPUTS: values and the four gradients, each allocated between two guard bands of its own, are written inside
their extent only, on both algorithms, with P = 777 (a partial block and a partial wave).

THE STREAM CONTRACT: "Every entry point of every family only enqueues on `stream`".  Forward and pullback (both
algorithms) run on a side stream after a filler and the copies of their inputs; the results are right after a
synchronisation of that stream alone."""
import ctypes

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests.test_parity_gpu import T, assert_close, tol
from tests.test_sample_smooth_clouds_gpu import P, _case, _check_pullback, _dev_args

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
B = 5
DTYPES = [(np.float32, torch.float32, "f32"), (np.float64, torch.float64, "f64")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _need(grid, n_points, nb, n_in, suf, group):
    a = np.asarray(grid, dtype=np.int64)
    f = getattr(dpr_amd.lib(), f"dpr_workspace_bytes_sample_smooth_clouds_ex_{suf}")
    return int(f(_lib.OP_PULLBACK, _lib.ALGO_TILED, _lib.flag_max_pose_group(group), n_in, len(grid),
                 a.ctypes.data_as(ctypes.c_void_p), n_points, nb))


def _problem(n_in, n_out, seed):
    return _case(n_in, n_out, nb=B, seed=seed)


def _guarded(shape, tdt, dev, grid_layout=False):
    """(view, whole): a tensor of `shape` (contiguous, or in the memory order of empty_grid) inside a buffer that
    holds GUARD bytes of 0xA5 on either side of it."""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=tdt).element_size()
    whole = torch.full((n * size + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    flat = whole[GUARD:GUARD + n * size].view(tdt)
    if grid_layout:
        return flat.view(tuple(reversed(shape))).permute(*reversed(range(len(shape)))), whole
    return flat.view(shape), whole


def _guards_intact(whole):
    return bool((whole[:GUARD] == GUARD_BYTE).all()) and bool((whole[-GUARD:] == GUARD_BYTE).all())


# ------------------------------------------------------------------ workspace
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt,suf", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_initial_contents_do_not_matter_and_nothing_is_written_outside(dev, group, npdt, tdt, suf, n_in, n_out):
    s, other = _problem(n_in, n_out, 4), _problem(n_in, n_out, 5)
    assert not np.array_equal(s["points"], other["points"]) and not np.array_equal(s["rot"], other["rot"])
    args, args_other = _dev_args(s, dev, npdt), _dev_args(other, dev, npdt)
    dv, dv_other = T(s["dv"].astype(npdt), dev), T(other["dv"].astype(npdt), dev)
    grid = s["grid"]
    need = _need(grid, P, B, n_in, suf, group)
    assert need > 0 and need % 256 == 0
    buf = torch.full((need + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    e = lambda *sh: torch.empty(sh, dtype=tdt, device=dev)
    outs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, tdt, dev), ds_dpoints=e(B, P, n_in),
                ds_drotation=e(B, n_in, n_out).transpose(1, 2), ds_dtranslation=e(B, n_out))
    kw = dict(algo="tiled", max_pose_group=group, workspace=ws, **outs)
    for pattern in ("zeros", "stale", "ones"):
        if pattern == "zeros":
            ws.zero_()
        elif pattern == "stale":
            dpr_amd.sample_smooth_clouds_pullback_(dv_other, *args_other, **kw)
        else:
            ws.fill_(0xFF)
        for t in outs.values():
            t.fill_(float("nan"))
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, **kw)
        torch.cuda.synchronize()
        assert _guards_intact(buf), f"{pattern}: bytes outside the {need} queried were overwritten"
        for name, t in outs.items():
            assert bool(torch.isfinite(t).all()), f"{pattern}: {name} holds NaN / Inf (or was not overwritten)"
        _check_pullback(pb, s["pb"], npdt, f"{pattern}: ")
    # one byte less than the query is refused, before any launch: the outputs keep their sentinel
    for t in outs.values():
        t.fill_(7.5)
    a = np.asarray(grid, dtype=np.int64)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    img, pts, rot, trans = args
    rot_cm = rot.transpose(1, 2).contiguous()
    d_rot = outs["ds_drotation"].transpose(1, 2)
    assert d_rot.is_contiguous()
    f = getattr(dpr_amd.lib(), f"dpr_sample_smooth_clouds_pullback_ex_{suf}")
    rc = f(None, _lib.ALGO_TILED, _lib.flag_max_pose_group(group), n_in, n_out, a.ctypes.data_as(ctypes.c_void_p), P,
           B, ptr(dv), ptr(img), ptr(pts), ptr(rot_cm), ptr(trans), ptr(outs["ds_dimage"]), ptr(outs["ds_dpoints"]),
           ptr(d_rot), ptr(outs["ds_dtranslation"]), ptr(ws), need - 1)
    assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_clouds_pullback_(dv, *args, algo="tiled", max_pose_group=group, workspace=ws[:need - 1])
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == 7.5).all()), f"a refused call wrote {name}"


# ------------------------------------------------------------------ outputs
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt,suf", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_outputs_are_written_inside_their_extent_only(dev, algo, npdt, tdt, suf, n_in, n_out):
    s = _problem(n_in, n_out, 4)
    assert s["points"].shape == (B, 777, n_in)
    args = _dev_args(s, dev, npdt)
    dv = T(s["dv"].astype(npdt), dev)
    values, w_values = _guarded((B, P), tdt, dev)
    d_img, w_img = _guarded(s["grid"] + (B,), tdt, dev, grid_layout=True)
    d_pts, w_pts = _guarded((B, P, n_in), tdt, dev)
    d_rot, w_rot = _guarded((B, n_in, n_out), tdt, dev)
    d_trans, w_trans = _guarded((B, n_out), tdt, dev)
    for t in (values, d_img, d_pts, d_rot, d_trans):
        t.fill_(float("nan"))
    v = dpr_amd.sample_smooth_clouds_(values, *args, algo="atomic")
    pb = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, algo=algo, ds_dimage=d_img, ds_dpoints=d_pts,
                                                ds_drotation=d_rot.transpose(1, 2), ds_dtranslation=d_trans)
    torch.cuda.synchronize()
    for name, whole in (("values", w_values), ("ds_dimage", w_img), ("ds_dpoints", w_pts), ("ds_drotation", w_rot),
                        ("ds_dtranslation", w_trans)):
        assert _guards_intact(whole), f"{algo}: bytes around {name} were overwritten"
    assert v.data_ptr() == values.data_ptr() and pb.image.data_ptr() == d_img.data_ptr()
    assert_close(v, s["values"].astype(npdt), tol(npdt, "points"), "values")
    _check_pullback(pb, s["pb"], npdt, f"{algo}: ")


# ------------------------------------------------------------------ stream
@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2)])
def test_runs_on_the_callers_stream(dev, n_in, n_out):
    """The inputs start as NaN; on a side stream a filler, the copies of the real inputs, the calls (forward, both
    pullback algorithms).  A launch or zeroing on another stream would not wait for them; only the side stream is
    synchronised before the results are read.  (Can pass by luck of timing, never fail by it.)"""
    s = _problem(n_in, n_out, 4)
    staged = _dev_args(s, dev, np.float32) + [T(s["dv"].astype(np.float32), dev)]
    inp = [torch.full_like(t, float("nan")) for t in staged]
    inp[0] = dpr_amd.to_grid_layout(inp[0])
    e = lambda *sh: torch.full(sh, float("nan"), device=dev)
    values = e(B, P)
    grads = {a: dict(ds_dimage=dpr_amd.empty_grid(s["grid"], B, torch.float32, dev).fill_(float("nan")),
                     ds_dpoints=e(B, P, n_in), ds_drotation=e(B, n_in, n_out).transpose(1, 2),
                     ds_dtranslation=e(B, n_out)) for a in ("atomic", "tiled")}
    ws = torch.empty(_need(s["grid"], P, B, n_in, "f32", 2), dtype=torch.uint8, device=dev)
    a = torch.randn(4096, 4096, device=dev)
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(4):  # (a few milliseconds on the side stream)
            torch.matmul(a, a, out=b)
        for dst, src in zip(inp, staged):
            dst.copy_(src, non_blocking=True)
        dpr_amd.sample_smooth_clouds_(values, *inp[:4])
        pb = {"atomic": dpr_amd.sample_smooth_clouds_pullback_(inp[4], *inp[:4], algo="atomic", **grads["atomic"]),
              "tiled": dpr_amd.sample_smooth_clouds_pullback_(inp[4], *inp[:4], algo="tiled", max_pose_group=2,
                                                              workspace=ws, **grads["tiled"])}
    side.synchronize()
    assert_close(values, s["values"].astype(np.float32), tol(np.float32, "points"), "side stream: values")
    for algo, g in pb.items():
        _check_pullback(g, s["pb"], np.float32, f"side stream: {algo} ")
