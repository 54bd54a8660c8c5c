"""Every op family beyond the core raster / pullback, held to the sentence of include/dpr.h that
tests/test_parity_gpu.py::test_runs_on_the_callers_stream_and_in_hip_graphs holds the core to: "every entry point of
every family only enqueues on `stream`, and can be captured into a HIP graph" -- no synchronising call, no
allocation, no launch or memset on another stream, no global state.  Since the split into csrc/dpr_api_*.hip every
family has a driver of its own, with its own memsets, pose loops, group loops and sort calls.

Per case -- each algorithm a family has, and the flag sets and shapes of tests/workspace_cases.py behind which a
driver has zeroing or group loops of its own (3-D chunk lists, local binning, pose groups, KEEP / REUSE) -- forward and pullback (the forward alone where there is no
pullback; a pullback that lacks the forward's algorithm runs the one the family pairs it with, Family.algos), the
shapes of tests/workspace_cases.py, preallocated outputs, the caller's workspace, fp32:

  side stream   The input buffers start as NaN.  On a non-default stream: a few milliseconds of matrix products, the
                copies of the real inputs (device to device and asynchronous, from buffers staged beforehand: the host
                does not wait, and reaches the driver while the filler is still running), the calls.  After
                side.synchronize() the results match the reference.  A launch or zeroing the driver put on any other
                stream would not wait for the filler and the copies: it reads NaN inputs, or its zeroes land behind
                the kernels they were meant to precede.  THIS CHECK CAN PASS BY LUCK OF TIMING AND CAN NEVER FAIL
                BY IT: work on a wrong stream that happens to run late enough is not seen.  The graph test is the
                one that cannot be lucky.
  graph         One warm-up on the side stream, then the same calls captured with torch.cuda.graph(graph,
                stream=side): one stream, no fork inside the capture.  A driver that synchronises, allocates or
                launches on another stream makes the capture raise.  New point, pose and image contents go into the
                same buffers, the outputs are filled with NaN, the graph is replayed, and the results match the
                reference of the new contents; then the first contents again and a second replay.  (What this found:
                the memset nodes of a captured hipMemsetAsync fill with stale host bytes on a replay -- the channel
                families' graphs on the first, others from the second on.  The drivers now zero with a kernel,
                zero_async of csrc/dpr_tiled.h.)
  threads       Four host threads, each with its own stream, buffers and workspace, run smooth TILED, smooth clouds
                TILED, channels TILED and ORDERED at the same time (ctypes drops the GIL during a call); one of them
                provokes a DprError.  Every thread gets its own results; dpr_last_error() is seen by that thread only.
"""
import threading

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests import data as D
from tests.test_parity_gpu import assert_close
from tests.workspace_cases import (FAMILIES, FLAGS, G2, G3, P_CHUNKS, P_ORDERED, P_SMALL, QUERY_OF, TDT, problem, reference,
                                   tolerance)

gpu = pytest.mark.gpu
DT = "f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _cases():
    """(family, algorithm, flag set of tests/workspace_cases.py, n_in, grid, P, B)"""
    cases = []
    for family, fam in FAMILIES.items():
        for algo in fam.algos:
            P = P_ORDERED if algo == "ordered" else P_SMALL
            cases.append((family, algo, "", 3, G3, P, 3))
    # drivers with zeroing or group loops of their own behind one algorithm name
    cases += [("core", "chunked", "", 3, G2, P_CHUNKS, 3),      # 2-D DPR_ALGO_CHUNKED
              ("core", "chunked", "", 3, G3, P_SMALL, 4),       # 3-D chunk lists (build_lists; no pullback of its own)
              ("core", "tiled", "local", 3, G3, P_SMALL, 3),    # bin_points_local: a zeroing per pose copy
              ("core", "tiled", "mpg1", 3, G3, P_SMALL, 3),     # one pose per group
              ("core", "tiled", "mpg2", 3, G2, P_SMALL, 3),     # groups of 2 + 1 poses
              ("core", "tiled", "sharing", 3, G3, P_SMALL, 3),  # KEEP forward, REUSE pullback
              ("smooth_clouds", "tiled", "mpg2", 3, G3, P_SMALL, 3)]  # groups of 2 + 1 clouds
    return cases


CASES = _cases()
IDS = [f"{f}-{a}{'+' + fl if fl else ''}-{len(g)}d-B{B}" for f, a, fl, _n, g, _P, B in CASES]
ARGS = "family,algo,flags,n_in,grid,P,B"
# the one refusal among the queries of these cases: 3-D DPR_ALGO_CHUNKED has no residual pullback
NO_RESIDUAL = ("core", "chunked", 3)


class Calls:
    """The calls of one case on device buffers that stay where they are."""

    def __init__(self, dev, family, algo, flags, n_in, grid, P, B):
        self.dev, self.family, self.fam, self.shape = dev, family, FAMILIES[family], (family, n_in, grid, P, B, DT)
        self.flags, self.pair = FLAGS[flags], flags == "sharing"
        p = self.problem(0)
        need, self.ops = 0, []
        for op in self.fam.ops:
            if op == "raster":  # (the sampling forwards run on DPR_ALGO_ATOMIC only)
                a = "atomic" if family in ("sample", "sample_smooth") else algo
            else:
                a = self.fam.algos[algo]
            if op == "residual_pullback" and ((family, algo, len(grid)) == NO_RESIDUAL or flags):
                continue  # (raster_residual_pullback_ has no max_pose_group argument; the pair runs the plain pullback)
            need = max(need, QUERY_OF[family](op, a, flags, n_in, grid, P, B, TDT[DT]))  # (a refusal raises)
            self.ops.append((op, a))
        assert [op for op, _a in self.ops][:1] == ["raster"] and len(self.ops) >= min(2, len(self.fam.ops))
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self.inp = self.fam.to_device(p, dev)
        self.out = {op: self.fam.outputs(op, p, dev) for op, _a in self.ops}
        self.staged = {}

    def problem(self, seed):
        return problem(*self.shape, seed)

    def poison(self):
        for t in self.inp.values():
            t.fill_(float("nan"))
        self.poison_outputs()

    def poison_outputs(self):
        for outs in self.out.values():
            for t in outs.values():
                t.fill_(float("nan"))

    def stage(self, *seeds):
        """the contents of `seeds` on the device, in buffers of their own (blocking copies from the host)"""
        for seed in seeds:
            self.staged[seed] = self.fam.to_device(self.problem(seed), self.dev)
        torch.cuda.synchronize()

    def load(self, seed):
        """staged contents into the buffers the calls read: asynchronous device-to-device copies on the current stream"""
        for k, t in self.inp.items():
            t.copy_(self.staged[seed][k], non_blocking=True)

    def run(self):
        if self.pair:
            kw = dict(algo="tiled", workspace=self.ws)
            poses = self.fam.poses(self.inp)
            dpr_amd.raster_(self.out["raster"]["out"], *poses, keep_binning=True, **kw)
            dpr_amd.raster_pullback_(self.inp["g"], *poses, reuse_binning=True, **kw,
                                     **{f"ds_d{k}": v for k, v in self.out["pullback"].items()})
            return
        for op, a in self.ops:
            self.fam.call(op, a, self.flags, self.inp, self.out[op], self.ws)

    def check(self, seed, what):
        for op, _a in self.ops:
            ref = reference(self.shape[0], op, *self.shape[1:], seed)
            for name, got in self.out[op].items():
                assert bool(torch.isfinite(got).all()), f"{what}: {op} {name} holds NaN"
                assert_close(got, ref[name], tolerance(self.family, DT, name), f"{what}: {op} {name}")


def filler(dev):
    a = torch.randn(4096, 4096, device=dev)
    b = torch.empty_like(a)
    return lambda: [torch.matmul(a, a, out=b) for _ in range(4)]  # (a few milliseconds on the stream it is called on)


@gpu
@pytest.mark.parametrize(ARGS, CASES, ids=IDS)
def test_runs_on_the_callers_stream(dev, family, algo, flags, n_in, grid, P, B):
    """(can pass by luck of timing, can never fail by it: see the module docstring)"""
    c = Calls(dev, family, algo, flags, n_in, grid, P, B)
    c.poison()
    c.stage(0)
    busy = filler(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        busy()
        done.record(side)
        c.load(0)
        c.run()
        still_busy = not done.query()  # (the host is through the driver: is the filler in front of it still running?)
    side.synchronize()
    print(f"filler still running when the calls had been enqueued: {still_busy}")
    c.check(0, "side stream")


@gpu
@pytest.mark.parametrize(ARGS, CASES, ids=IDS)
def test_is_captured_into_a_hip_graph_and_replayed_on_new_contents(dev, family, algo, flags, n_in, grid, P, B):
    c = Calls(dev, family, algo, flags, n_in, grid, P, B)
    c.stage(0, 2)
    c.load(0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c.run()  # warm-up outside the capture
    side.synchronize()
    c.check(0, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c.run()
    c.load(2)
    c.poison_outputs()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    c.check(2, "graph replay on new contents")
    c.load(0)  # (and once more: a node that keeps host state of the capture goes wrong on a later replay)
    c.poison_outputs()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    c.check(0, "second replay, on the first contents")


@gpu
def test_concurrent_host_threads_of_four_families(dev):
    """In the shape of tests/test_parity_gpu.py::test_concurrent_host_threads_on_their_own_streams: thread 0 hands a
    DPR_ALGO_ATOMIC forward a KEEP flag after its own work; its message stays on its own thread."""
    plan = [("smooth", "tiled", P_SMALL), ("smooth_clouds", "tiled", P_SMALL), ("channels", "tiled", P_SMALL),
            ("core", "ordered", P_ORDERED)]
    results, errors, messages = [None] * len(plan), [], [None] * len(plan)

    def worker(i):
        try:
            family, algo, P = plan[i]
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                c = Calls(dev, family, algo, "", 3, G3, P, 3)
                c.stage(0)
                c.load(0)
                for _ in range(3):  # keep the threads overlapping for a while
                    c.poison_outputs()
                    c.run()
                if i == 0:
                    with pytest.raises(dpr_amd.DprError):
                        dpr_amd.raster_(c.out["raster"]["out"].clone(), *c.fam.poses(c.inp), algo="atomic",
                                        keep_binning=True,
                                        workspace=torch.empty(1 << 20, dtype=torch.uint8, device=dev))
            stream.synchronize()
            messages[i] = _lib.last_error()
            results[i] = c
        except Exception as e:  # surfaced in the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(plan))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, c in enumerate(results):
        c.check(0, f"thread {i} ({plan[i][0]} {plan[i][1]})")
    assert messages[0] and all(m == "" for m in messages[1:]), messages


@gpu
def test_a_sort_of_more_than_2_pow_20_keys_is_refused_under_capture(dev, oracle):
    """The one exception of the stream contract (include/dpr.h): above 2^20 keys rocPRIM's radix sort clears its
    histograms with hipMemsetAsync, whose graph nodes are not replayed reliably, so csrc/dpr_sort.hip refuses the
    sort on a capturing stream -- DPR_ALGO_ORDERED's forward here, P = 2^20 + 1.  The same call outside a capture
    runs and gives the oracle's image, and one key fewer is captured and replayed."""
    grid, B = (40, 24), 1
    for P, refused in (((1 << 20) + 1, True), (1 << 20, False)):
        d = D.make(n_points=P, n_in=2, n_out=2, batch=B, grid_n=grid, seed=77, dtype=np.float32)
        args = [torch.as_tensor(a, device=dev) for a in (d.points, d.rotations, d.translations, d.backgrounds, d.weights)]
        out = dpr_amd.empty_grid(grid, B, torch.float32, dev)
        ws = torch.empty(dpr_amd.workspace_bytes("raster", grid, P, B, 2, torch.float32, "ordered"), dtype=torch.uint8,
                         device=dev)
        ref = oracle.raster(grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights, dtype=np.float32)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            dpr_amd.raster_(out, *args, algo="ordered", workspace=ws)
        side.synchronize()
        assert_close(out, ref, tolerance("core", DT, "out"), f"P = {P}, outside a capture")
        graph = torch.cuda.CUDAGraph()
        if refused:
            with pytest.raises(dpr_amd.DprError, match="capturing"):
                with torch.cuda.graph(graph, stream=side):
                    dpr_amd.raster_(out, *args, algo="ordered", workspace=ws)
        else:
            with torch.cuda.graph(graph, stream=side):
                dpr_amd.raster_(out, *args, algo="ordered", workspace=ws)
            for _ in range(2):
                out.fill_(float("nan"))
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                assert_close(out, ref, tolerance("core", DT, "out"), f"P = {P}, replayed")
