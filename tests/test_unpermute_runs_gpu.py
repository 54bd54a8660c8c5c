"""The run-ordered un-permute of the tiled pullback (k_scatter_wc_runs -> k_unpermute_runs): one pose through
the write-combining scatter leaves the un-permute's map in SORTED order, the un-permute gathers whole record runs
and puts them back in original order through an LDS stage.

The kernel pair is a pure permutation of what k_tile_gather computed per record, so beyond oracle parity (the
tolerances of tests/test_parity_gpu.py) everything here is held to ==, on the bytes:
  * shuffling the cloud shuffles the point gradients (the property a wrong map breaks),
  * the plain pullback equals the KEEP forward + REUSE pullback,
  * point_weight_grad=False leaves ds_dpoints as it was and allocates no ds_dpoint_weight,
  * rejected points (no in-range voxel) own no sorted position and leave with exact zeros.
Shapes: 64^3 (32 tiles) and 128^2 (16 tiles), P around the scatter's sub-chunk (4096 points fp32, 2048 fp64):
a partial round, an exact one, ragged ones, and 2 * 256 * 4096 + 5 points -- the plan cuts the cloud into at most
256 slices of whole sub-chunks, so there every slice holds more than one round and the last one is ragged.
"""
import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
GRIDS = [(3, 3, 64), (3, 2, 128)]  # (n_in, n_out, grid_n): 32 tiles of 64 x 16 x 8, 16 tiles of 32 x 32
POINT_COUNTS = [1, 4095, 4096, 4097, 3 * 4096 + 17, 2 * 256 * 4096 + 5]
# margin (in voxels) by which a point must miss the grid to count as rejected in the test's own fp64 projection:
# far above the rounding of the fp32 projection (~1e-5 voxels on these grids), far below the spread of the cloud
REJECT_MARGIN = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def same_bytes(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def surely_rejected(d, b=0):
    """Points without an in-range voxel under pose b (dpr_device.h, ref_and_deltas: c in (-1, n] on every axis
    is accepted), decided in fp64 with REJECT_MARGIN to spare."""
    pts = d.points.astype(np.float64)
    proj = pts @ d.rotations[b].astype(np.float64).T + d.translations[b].astype(np.float64)
    n = np.asarray(d.grid, dtype=np.float64)
    c = (proj + 1.0) * (n / 2.0) - 0.5
    return np.any((c < -1.0 - REJECT_MARGIN) | (c > n + REJECT_MARGIN), axis=1)


def dev_args(d, dev, with_pw, perm=None):
    pts = d.points if perm is None else d.points[perm]
    pw = None if not with_pw else (d.point_weights if perm is None else d.point_weights[perm])
    return (T(pts, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev), T(d.weights, dev),
            T(pw, dev))


def check_oracle(oracle, d, pb, npdt, with_pw):
    pw = d.point_weights if with_pw else None
    ref = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, pw, dtype=npdt)
    assert_close(pb.points, ref.points, tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight, ref.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
    assert_close(pb.rotation, ref.rotation, tol(npdt, "pose"), "ds_drotation")
    assert_close(pb.translation, ref.translation, tol(npdt, "pose"), "ds_dtranslation")
    assert_close(pb.background, ref.background, tol(npdt, "pose"), "ds_dbackground")
    assert_close(pb.out_weight, ref.out_weight, tol(npdt, "pose"), "ds_dout_weight")


def check_shuffle(d, dev, g, pb, with_pw, seed, **kw):
    perm = np.random.default_rng(seed).permutation(d.n_points)
    pb_s = dpr_amd.raster_pullback_(g, *dev_args(d, dev, with_pw, perm), algo="tiled", **kw)
    iperm = torch.as_tensor(perm, device=dev)
    assert same_bytes(pb_s.points, pb.points[iperm]), "ds_dpoints of the shuffled cloud"
    assert same_bytes(pb_s.point_weight, pb.point_weight[iperm]), "ds_dpoint_weight of the shuffled cloud"


def check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected):
    """Assertions 1-4 of the module docstring on the single-pose cloud `d`."""
    args = dev_args(d, dev, with_pw)
    g = grid_to_dev(d.ds_dout, dev)
    pb = dpr_amd.raster_pullback_(g, *args, algo="tiled")
    check_oracle(oracle, d, pb, npdt, with_pw)
    check_shuffle(d, dev, g, pb, with_pw, seed=d.n_points)
    # KEEP forward + REUSE pullback
    need = max(dpr_amd.workspace_bytes(op, d.grid, d.n_points, 1, d.n_in, tdt, "tiled", sharing=True)
               for op in ("raster", "pullback"))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, 1, tdt, dev)
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
    pb_r = dpr_amd.raster_pullback_(g, *args, algo="tiled", workspace=ws, reuse_binning=True)
    assert same_bytes(pb_r.points, pb.points), "ds_dpoints: KEEP / REUSE against the plain pullback"
    assert same_bytes(pb_r.point_weight, pb.point_weight), "ds_dpoint_weight: KEEP / REUSE against the plain pullback"
    # without the point-weight gradient, plain and paired
    pb_n = dpr_amd.raster_pullback_(g, *args, algo="tiled", point_weight_grad=False)
    assert pb_n.point_weight is None
    assert same_bytes(pb_n.points, pb.points), "ds_dpoints with point_weight_grad=False"
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
    pb_rn = dpr_amd.raster_pullback_(g, *args, algo="tiled", workspace=ws, reuse_binning=True,
                                     point_weight_grad=False)
    assert pb_rn.point_weight is None
    assert same_bytes(pb_rn.points, pb.points), "ds_dpoints with point_weight_grad=False, KEEP / REUSE"
    # rejected points: exact zeros
    rej = surely_rejected(d)
    if want_rejected:
        assert rej.any(), "the cloud should hold points outside the grid"
    if rej.any():
        r = torch.as_tensor(np.nonzero(rej)[0], device=dev)
        for x in (pb, pb_r):
            assert not bool(x.points[r].view(-1).to(torch.float64).abs().max() > 0), "rejected points: ds_dpoints"
            assert not bool(x.point_weight[r].to(torch.float64).abs().max() > 0), "rejected points: ds_dpoint_weight"
    return pb


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
@pytest.mark.parametrize("n_points", POINT_COUNTS)
def test_round_shapes(oracle, dev, n_points, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """0.4 N(0, I): several per cent of the cloud misses the grid.  (One point alone may well land inside: the
    cloud is asked for a rejected point from 4095 points on.)"""
    d = D.make(n_points=n_points, n_in=n_in, n_out=n_out, batch=1, grid_n=grid_n, seed=100 + n_out, dtype=npdt)
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=n_points >= 4095)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_dense_cloud_with_split_tiles(oracle, dev, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """0.05 N(0, I), 2e5 points: the central tiles hold far more records than the split threshold (4096 in
    3-D, 2048 in 2-D), so the gradient records the un-permute reads were written by the parts of split tiles."""
    d = D.make(n_points=200_000, n_in=n_in, n_out=n_out, batch=1, grid_n=grid_n, seed=7, dtype=npdt)
    d.points *= 0.125  # 0.4 -> 0.05
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=False)


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_every_point_rejected(oracle, dev, n_in, n_out, grid_n, npdt, tdt):
    d = D.make(n_points=5000, n_in=n_in, n_out=n_out, batch=1, grid_n=grid_n, seed=9, dtype=npdt)
    d.points += 10.0
    assert surely_rejected(d).all()
    pb = check_everything(oracle, dev, d, npdt, tdt, True, want_rejected=True)
    assert not bool(pb.points.abs().max() > 0) and not bool(pb.point_weight.abs().max() > 0)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_pose_group_keeps_the_point_order_map(oracle, dev, npdt, tdt, with_pw):
    """Four poses on 64^3 form a pose group: slot_of[p] and k_unpermute, as before."""
    d = D.make(n_points=3 * 4096 + 17, n_in=3, n_out=3, batch=4, grid_n=64, seed=11, dtype=npdt)
    g = grid_to_dev(d.ds_dout, dev)
    pb = dpr_amd.raster_pullback_(g, *dev_args(d, dev, with_pw), algo="tiled")
    check_oracle(oracle, d, pb, npdt, with_pw)
    check_shuffle(d, dev, g, pb, with_pw, seed=12)


@pytest.mark.parametrize("with_pw", [False, True])
def test_large_grid_keeps_the_point_order_map(oracle, dev, with_pw):
    """4096^2: 16384 tiles, beyond the write-combining scatter -- k_scatter, slot_of[p] and k_unpermute, as
    before.  (fp32 only: the 128 MB image of the fp64 case buys no other code path.)"""
    d = D.make(n_points=100_000, n_in=3, n_out=2, batch=1, grid_n=4096, seed=13, dtype=np.float32)
    g = grid_to_dev(d.ds_dout, dev)
    pb = dpr_amd.raster_pullback_(g, *dev_args(d, dev, with_pw), algo="tiled")
    check_oracle(oracle, d, pb, np.float32, with_pw)
    check_shuffle(d, dev, g, pb, with_pw, seed=14)


def test_reuse_without_a_matching_forward_is_nan(oracle, dev):
    """As test_reuse_binning_is_validated_on_the_device, on a shape of this file: the run-ordered un-permute
    fills NaN and reads nothing through a map no KEEP forward of this call pair wrote."""
    d = D.make(n_points=3 * 4096 + 17, n_in=3, n_out=3, batch=1, grid_n=64, seed=15, dtype=np.float32)
    args = dev_args(d, dev, True)
    g = grid_to_dev(d.ds_dout, dev)
    need = max(dpr_amd.workspace_bytes(op, d.grid, d.n_points, 1, 3, torch.float32, "tiled", sharing=True)
               for op in ("raster", "pullback"))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, 1, torch.float32, dev)
    isnan = lambda pb: all(bool(torch.isnan(x).all()) for x in pb)
    reuse = lambda *a: dpr_amd.raster_pullback_(g, *a, algo="tiled", workspace=ws, reuse_binning=True)
    assert isnan(reuse(*args))  # nothing was kept
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws)
    assert isnan(reuse(*args))  # a forward without keep_binning
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
    pb = reuse(*args)
    check_oracle(oracle, d, pb, np.float32, True)
    assert isnan(reuse(*args))  # consumed
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
    assert isnan(reuse(args[0], args[1], args[2] + 0.01, *args[3:]))  # kept for another pose
