"""Smooth sampling at the points of rigid bodies held to the two contracts of include/dpr.h, in the pattern of
tests/test_smooth_bodies_contract_gpu.py.

THE WORKSPACE CONTRACT: "The initial contents of the workspace do not matter: every piece of a layout is written by the
call before the call reads it.  The library writes only inside [workspace, workspace + workspace_bytes)."  The TILED
pullback runs on the interior view buf[4096 : 4096 + need] of a uint8 buffer whose two guard bands of 4096 bytes hold
0xA5, with `need` from dpr_workspace_bytes_sample_smooth_bodies_ex_* for the flags of the call, on three workspace
contents: zeros; stale (what a call with another cloud, other bodies and other poses left behind); every byte 0xFF (the
all-ones key, the largest index and count).  Afterwards the guards are unchanged and the four outputs, pre-filled with
NaN, are finite and match the reference -- for groups of one image, of two (2 + 2 + 1) and the default (all five).

THE STREAM CONTRACT: "Every entry point of every family only enqueues on `stream`, and can be captured into a HIP
graph".  Forward and pullback (both algorithms) run on a side stream after a filler and the copies of their inputs,
and are captured with torch.cuda.graph(graph, stream=side) -- one stream, no fork -- and replayed on new contents of
the same buffers, then on the first contents again."""
import ctypes

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests.test_parity_gpu import assert_close, tol
from tests.test_sample_smooth_bodies_gpu import _args, _check_pullback, _dv, _scase

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
SIZES = (100, 100, 100)  # P = 300 in K = 3 bodies
B = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _need(grid, P, nb, K, n_in, suf, group):
    a = np.asarray(grid, dtype=np.int64)
    f = getattr(dpr_amd.lib(), f"dpr_workspace_bytes_sample_smooth_bodies_ex_{suf}")
    return int(f(_lib.OP_PULLBACK, _lib.ALGO_TILED, _lib.flag_max_pose_group(group), n_in, len(grid),
                 a.ctypes.data_as(ctypes.c_void_p), P, nb, K))


def _problem(n_in, n_out, seed):
    return _scase(n_in, n_out, sizes=SIZES, B=B, order="shuffled", seed=seed)


# ------------------------------------------------------------------ workspace
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt,suf", [(np.float32, torch.float32, "f32"), (np.float64, torch.float64, "f64")])
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_initial_contents_do_not_matter_and_nothing_is_written_outside(dev, group, npdt, tdt, suf, n_in, n_out):
    s, other = _problem(n_in, n_out, 4), _problem(n_in, n_out, 5)
    assert not np.array_equal(s["points"], other["points"]) and not np.array_equal(s["rot"], other["rot"])
    args, args_other = _args(s, dev, npdt), _args(other, dev, npdt)
    args_other[2] = torch.roll(args_other[2], 7)  # other bodies
    dv, dv_other = _dv(s, dev, npdt), _dv(other, dev, npdt)
    P, K = s["P"], s["K"]
    need = _need(s["grid"], P, B, K, n_in, suf, group)
    assert need > 0 and need % 256 == 0
    buf = torch.full((need + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    band = torch.full((GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    e = lambda *sh: torch.empty(sh, dtype=tdt, device=dev)
    outs = dict(ds_dimage=dpr_amd.empty_grid(s["grid"], B, tdt, dev), ds_dpoints=e(P, n_in),
                ds_drotation=e(B, K, n_in, n_out).transpose(-1, -2), ds_dtranslation=e(B, K, n_out))
    kw = dict(algo="tiled", max_pose_group=group, workspace=ws, **outs)
    for pattern in ("zeros", "stale", "ones"):
        if pattern == "zeros":
            ws.zero_()
        elif pattern == "stale":
            dpr_amd.sample_smooth_bodies_pullback_(dv_other, *args_other, **kw)
        else:
            ws.fill_(0xFF)
        for t in outs.values():
            t.fill_(float("nan"))
        pb = dpr_amd.sample_smooth_bodies_pullback_(dv, *args, **kw)
        torch.cuda.synchronize()
        assert torch.equal(buf[:GUARD], band), f"{pattern}: bytes in front of the workspace were overwritten"
        assert torch.equal(buf[GUARD + need:], band), f"{pattern}: bytes behind the {need} queried were overwritten"
        for name, t in outs.items():
            assert bool(torch.isfinite(t).all()), f"{pattern}: {name} holds NaN / Inf (or was not overwritten)"
        _check_pullback(pb, s["pb"], npdt, f"{pattern}: ")
    # less than the query is refused, before any launch
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_bodies_pullback_(dv, *args, algo="tiled", max_pose_group=group, workspace=ws[:need - 256])


# ------------------------------------------------------------------ stream
class Calls:
    """Forward and pullback (both algorithms) on device buffers that stay where they are."""

    def __init__(self, dev, n_in, n_out):
        self.dev, self.n_in, self.n_out = dev, n_in, n_out
        s = _problem(n_in, n_out, 4)
        self.inp = _args(s, dev, np.float32, body_dtype=torch.int32)  # (int32: the calls make no copy of it)
        self.dv = _dv(s, dev, np.float32)
        P, K = s["P"], s["K"]
        e = lambda *sh: torch.empty(sh, device=dev)
        self.values = e(B, P).t()
        self.grads = {a: dict(ds_dimage=dpr_amd.empty_grid(s["grid"], B, torch.float32, dev), ds_dpoints=e(P, n_in),
                              ds_drotation=e(B, K, n_in, n_out).transpose(-1, -2), ds_dtranslation=e(B, K, n_out))
                      for a in ("atomic", "tiled")}
        self.ws = torch.empty(_need(s["grid"], P, B, K, n_in, "f32", 2), dtype=torch.uint8, device=dev)
        self.staged = {}

    def poison_inputs(self):
        for v in self.inp + [self.dv]:
            v.fill_(-1 if v.dtype == torch.int32 else float("nan"))

    def poison_outputs(self):
        for v in [self.values] + [t for g in self.grads.values() for t in g.values()]:
            v.fill_(float("nan"))

    def stage(self, *seeds):
        for seed in seeds:
            s = _problem(self.n_in, self.n_out, seed)
            self.staged[seed] = (_args(s, self.dev, np.float32, body_dtype=torch.int32), _dv(s, self.dev, np.float32))
        torch.cuda.synchronize()

    def load(self, seed):
        args, dv = self.staged[seed]
        for dst, src in zip(self.inp + [self.dv], args + [dv]):
            dst.copy_(src, non_blocking=True)

    def run(self):
        dpr_amd.sample_smooth_bodies_(self.values, *self.inp)
        self.pb = {"atomic": dpr_amd.sample_smooth_bodies_pullback_(self.dv, *self.inp, algo="atomic",
                                                                    **self.grads["atomic"]),
                   "tiled": dpr_amd.sample_smooth_bodies_pullback_(self.dv, *self.inp, algo="tiled", max_pose_group=2,
                                                                   workspace=self.ws, **self.grads["tiled"])}

    def check(self, seed, what):
        s = _problem(self.n_in, self.n_out, seed)
        assert_close(self.values, s["values"].astype(np.float32), tol(np.float32, "points"), f"{what}: values")
        for a, pb in self.pb.items():
            _check_pullback(pb, s["pb"], np.float32, f"{what}: {a} ")


def _filler(dev):
    a = torch.randn(4096, 4096, device=dev)
    b = torch.empty_like(a)
    return lambda: [torch.matmul(a, a, out=b) for _ in range(4)]  # (a few milliseconds on the stream it is called on)


@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2)])
def test_runs_on_the_callers_stream(dev, n_in, n_out):
    """The inputs start as NaN (body: -1); on a side stream a filler, the copies of the real inputs, the calls.  A
    launch or zeroing on another stream would not wait for them.  (Can pass by luck of timing, never fail by it.)"""
    c = Calls(dev, n_in, n_out)
    c.poison_inputs()
    c.poison_outputs()
    c.stage(4)
    busy = _filler(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        busy()
        c.load(4)
        c.run()
    side.synchronize()
    c.check(4, "side stream")


@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2)])
def test_is_captured_into_a_hip_graph_and_replayed_on_new_contents(dev, n_in, n_out):
    c = Calls(dev, n_in, n_out)
    c.stage(4, 5)
    c.load(4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c.run()  # warm-up outside the capture
    side.synchronize()
    c.check(4, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one stream, no fork
        c.run()
    for seed, what in ((5, "graph replay on new contents"), (4, "second replay, on the first contents")):
        c.load(seed)
        c.poison_outputs()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        c.check(seed, what)
