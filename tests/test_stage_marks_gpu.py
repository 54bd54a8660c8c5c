"""The stage-mark contract of DPR_ALGO_TILED: every walk of the pipeline (a pose, a pose group, a slab) records
one mark per stage of timing.py's table, on every branch -- a REUSE_BINNING pullback and the later poses of a
local batch, which bin nothing, record their three binning marks back to back.  `stage_times` folds the walks by
count and raises when the count is off; bench.py and the tools rely on that.  No time is asserted."""
import math

import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D

pytestmark = pytest.mark.gpu

STAGES = dpr_amd._pkg.timing.STAGES

N_POINTS = 20_000
SHAPES = [(3, 3, 64), (2, 2, 128)]  # n_in, n_out, grid_n
BATCHES = [1, 3]


def _problem(n_in, n_out, grid_n, batch):
    dev = torch.device("cuda:0")
    d = D.make(n_points=N_POINTS, n_in=n_in, n_out=n_out, batch=batch, grid_n=grid_n, seed=5, dtype=np.float32)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    args = (to(d.points), to(d.rotations), to(d.translations), to(d.backgrounds), to(d.weights),
            to(d.point_weights))
    g = dpr_amd.to_grid_layout(to(d.ds_dout))
    out = dpr_amd.empty_grid(d.grid, batch, torch.float32, dev)
    return d, args, g, out


def _check(times, op, name):
    assert list(times) == STAGES[(op, name)] + ["total"]
    for stage, ms in times.items():
        assert math.isfinite(ms) and ms >= 0, f"{stage}: {ms}"


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n_in,n_out,grid_n", SHAPES)
@pytest.mark.parametrize("op,name", [("raster", "tiled"), ("pullback", "tiled"), ("raster", "tiled_local"),
                                     ("pullback", "tiled_local")])
def test_tiled_calls_mark_every_stage_of_the_table(op, name, n_in, n_out, grid_n, batch):
    d, args, g, out = _problem(n_in, n_out, grid_n, batch)
    kw = dict(algo="tiled", coherent_points=name == "tiled_local")
    if op == "raster":
        call = lambda: dpr_amd.raster_(out, *args, **kw)
    else:
        call = lambda: dpr_amd.raster_pullback_(g, *args, **kw)
    _check(dpr_amd.stage_times(call, op, name, reps=2), op, name)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n_in,n_out,grid_n", SHAPES)
def test_a_reuse_pullback_marks_every_stage_of_the_table(n_in, n_out, grid_n, batch):
    d, args, g, out = _problem(n_in, n_out, grid_n, batch)
    ws = torch.empty(max(dpr_amd.workspace_bytes(op, d.grid, N_POINTS, batch, n_in, torch.float32, "tiled",
                                                 sharing=True) for op in ("raster", "pullback")),
                     dtype=torch.uint8, device=out.device)
    fwd = lambda: dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
    bwd = lambda: dpr_amd.raster_pullback_(g, *args, algo="tiled", workspace=ws, reuse_binning=True)
    _check(dpr_amd.stage_times(bwd, "pullback", "tiled", reps=2, prepare=fwd), "pullback", "tiled")
