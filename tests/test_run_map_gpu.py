"""The per-run un-permute map of the tiled pullback on the GPU (csrc/dpr_run_map.h: k_scatter_wc_runs keeps an owner
word with a run-start bit per sorted position and ONE record slot per run -- a run being the records of one tile
inside one segment of 64 sorted positions --, k_unpermute_runs rebuilds every slot from the start bits of the segment).

The kernel pair is a pure permutation of what k_tile_gather computed per record, so every case is held to the four
statements of tests/test_unpermute_runs_gpu.py (its check_everything, with the helpers and tolerances of
tests/test_parity_gpu.py): oracle parity, == on the bytes of ds_dpoints / ds_dpoint_weight under a shuffle of the
cloud, == between the plain pullback and KEEP forward + REUSE pullback, exact zeros for rejected points.

Beyond random clouds around the sub-chunk size (4096 points fp32, 2048 fp64), clouds are CONSTRUCTED at chosen grid
coordinates (`place`: the points whose projection under the pose is the wanted one), on 64^3 (32 tiles of 64 x 16 x 8)
and 128^2 (16 tiles of 32 x 32):
  (a) all points inside one tile: one run per sub-chunk,
  (b) points dealt round-robin over all tiles: every sub-chunk has as many runs as there are tiles,
  (c) a whole sub-chunk of rejected points between two ordinary ones,
  (d) the points of a sub-chunk alternately valid and rejected,
  (e) the most runs a sub-chunk of a random cloud will see, more tiles' runs than half its positions: 2 S + 3 points
      uniform over 512 x 256 x 192 (3072 tiles, ~2240 of them met by 4096 points) in fp32 and over 256^3 (2048 tiles,
      ~1300 met by 2048 points) in fp64 -- 35 and 40 runs per segment of 64 against 19 on the benchmark's cloud; the
      count is asserted.  (A map with one table for the whole sub-chunk, the first half of it fetched ahead, was
      measured and not built, profiles/run_map_per_run.md; the case is the one that passed its half.)
  (f) every position the start of a run: fp64 on 256^3 has as many tiles as a sub-chunk has points, dealt round-robin.
"""
import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests.test_unpermute_runs_gpu import check_everything, surely_rejected

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
GRIDS = [(3, 3, 64), (3, 2, 128)]  # (n_in, n_out, grid_n)
POINT_COUNTS = [1, 4095, 4096, 4097, 3 * 4096 + 17]
TILE = {3: (64, 16, 8), 2: (32, 32)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def sub_chunk(npdt):
    return 4096 if npdt == np.float32 else 2048


def place(d, c):
    """Put the points of the single-pose cloud `d` where they project to voxel coordinates `c` (P x n_out; voxel i
    spans [i, i + 1)): rows of the rotation are orthonormal, so p = (u - t) R projects to u."""
    n = np.asarray(d.grid, dtype=np.float64)
    u = (np.asarray(c, dtype=np.float64) + 0.5) * (2.0 / n) - 1.0
    p = (u - d.translations[0].astype(np.float64)) @ d.rotations[0].astype(np.float64)
    d.points = np.ascontiguousarray(p, dtype=d.points.dtype)


def tiles_of(d):
    """(tiles per axis, tile extents) of the grid of `d`."""
    ext = np.asarray(TILE[d.n_out])
    return -(-np.asarray(d.grid) // ext), ext


def in_tile(rng, d, tile_ids):
    """Voxel coordinates in the middle half of the given tiles (column-major ids): off every tile edge by a
    quarter of the tile, far beyond the rounding of the projection."""
    nt, ext = tiles_of(d)
    t = np.asarray(tile_ids)
    c = np.empty((len(t), d.n_out))
    for a in range(d.n_out):
        c[:, a] = (t % nt[a]) * ext[a] + ext[a] * rng.uniform(0.25, 0.75, size=len(t))
        t = t // nt[a]
    return c


def make(n_points, n_in, n_out, grid_n, seed, npdt):
    return D.make(n_points=n_points, n_in=n_in, n_out=n_out, batch=1, grid_n=grid_n, seed=seed, dtype=npdt)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
@pytest.mark.parametrize("n_points", POINT_COUNTS)
def test_random_clouds_around_the_sub_chunk(oracle, dev, n_points, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """0.4 N(0, I): several per cent of the cloud misses the grid (asked for from 4095 points on)."""
    d = make(n_points, n_in, n_out, grid_n, 200 + n_out, npdt)
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=n_points >= 4095)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_one_tile_one_run_per_sub_chunk(oracle, dev, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """(a)"""
    S = sub_chunk(npdt)
    d = make(2 * S + 3, n_in, n_out, grid_n, 21, npdt)
    nt, _ = tiles_of(d)
    place(d, in_tile(np.random.default_rng(22), d, np.full(d.n_points, int(np.prod(nt)) // 2 + 1)))
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=False)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_round_robin_over_all_tiles(oracle, dev, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """(b)"""
    S = sub_chunk(npdt)
    d = make(2 * S + 3, n_in, n_out, grid_n, 23, npdt)
    nt, _ = tiles_of(d)
    place(d, in_tile(np.random.default_rng(24), d, np.arange(d.n_points) % int(np.prod(nt))))
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=False)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_a_sub_chunk_of_rejected_points_between_two_ordinary_ones(oracle, dev, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """(c)"""
    S = sub_chunk(npdt)
    d = make(3 * S, n_in, n_out, grid_n, 25, npdt)
    d.points[S:2 * S] += 10.0
    assert surely_rejected(d)[S:2 * S].all()
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=True)


@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid_n", GRIDS)
def test_valid_and_rejected_points_alternating(oracle, dev, n_in, n_out, grid_n, npdt, tdt, with_pw):
    """(d)"""
    S = sub_chunk(npdt)
    d = make(2 * S + 5, n_in, n_out, grid_n, 27, npdt)
    d.points[1::2] += 10.0
    assert surely_rejected(d)[1::2].all()
    check_everything(oracle, dev, d, npdt, tdt, with_pw, want_rejected=True)


@pytest.mark.parametrize("npdt,tdt,grid", [(np.float32, torch.float32, (512, 256, 192)),
                                           (np.float64, torch.float64, (256, 256, 256))])
def test_more_tiles_met_than_half_the_positions(oracle, dev, npdt, tdt, grid):
    """(e)"""
    S = sub_chunk(npdt)
    d = make(2 * S + 3, 3, 3, grid, 29, npdt)
    rng = np.random.default_rng(30)
    c = rng.uniform(0.5, np.asarray(grid) - 1.5, size=(d.n_points, 3))
    place(d, c)
    nt, ext = tiles_of(d)
    assert int(np.prod(nt)) <= 4096, "the write-combining scatter and its sorted map stop at 4096 tiles"
    tile = np.floor(c).astype(np.int64) // ext
    ids = tile[:, 0] + nt[0] * (tile[:, 1] + nt[1] * tile[:, 2])
    runs = max(len(np.unique(ids[g * S:(g + 1) * S])) for g in range(2))
    # (points next to a tile face may fall on either side of it on the device: a few dozen of the S at most)
    assert runs > S // 2 + 100, f"{runs} tiles met by a sub-chunk of {S} points: no more than half its positions"
    check_everything(oracle, dev, d, npdt, tdt, True, want_rejected=False)


def test_every_position_starts_a_run(oracle, dev):
    """fp64 on 256^3: as many tiles as a sub-chunk has points (2048), the points dealt round-robin -- every point of a
    sub-chunk in a tile of its own, 64 runs in every segment."""
    S = sub_chunk(np.float64)
    d = make(2 * S + 3, 3, 3, (256, 256, 256), 31, np.float64)
    nt, _ = tiles_of(d)
    assert int(np.prod(nt)) == S
    place(d, in_tile(np.random.default_rng(32), d, np.arange(d.n_points) % S))
    check_everything(oracle, dev, d, np.float64, torch.float64, True, want_rejected=False)
