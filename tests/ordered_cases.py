"""Generated inputs of the DPR_ALGO_ORDERED tests (tests/test_ordered_host.py, tests/test_ordered_gpu.py): small,
finite clouds that exercise rejected points, reference cells at -1, neighbours dropped one by one, points on cell
centres and faces, one crowded cell, axes of length 1, and weights of both signs spanning more than 2^10.  The same
clouds go to the host program (tests/ordered_host_check.cpp) as files and to the GPU as tensors."""
import struct
from types import SimpleNamespace

import numpy as np

from tests import data as D

KINDS = ("overhang", "centres_faces", "one_cell")
# (n_in, n_out) -> the awkward grid the issue names for that output dimension
NASTY_GRIDS = {1: (6,), 2: (1, 6), 3: (7, 9, 5), 4: (3, 4, 2, 5)}


def _isometries(rng, batch, n_out, n_in):
    if n_in > 3 or n_out > n_in:
        return D.random_isometries(rng, batch, n_out, n_in)
    return D.random_rotations(rng, batch, n_in)[:, :n_out, :]


def make(kind, n_in, n_out, n_points, batch, grid, seed=0, dtype=np.float32):
    """A cloud of `kind` with nasty weights: random-normal point weights times 2^U(-6, 6), a negative out_weight
    on pose 0, non-zero backgrounds.  `grid`: an int (cubic) or a tuple."""
    assert kind in KINDS
    rng = np.random.default_rng(seed)
    grid = tuple(grid) if isinstance(grid, (tuple, list)) else (int(grid),) * n_out
    assert len(grid) == n_out
    rot = _isometries(rng, batch, n_out, n_in)
    trans = 0.1 * rng.normal(size=(batch, n_out))
    if kind == "overhang":
        # sigma 0.75 on [-1, 1]: a fifth of the coordinates fall off the grid on either side, many by less than a cell
        points = 0.75 * rng.normal(size=(n_points, n_in))
    elif kind == "centres_faces":
        # axis-aligned poses without translation: coord = (p + 1) * n / 2 is k + 1/2 (a centre) or k (a face), for k
        # from one cell below the grid to one cell above it
        rot = np.broadcast_to(np.eye(n_out, n_in), (batch, n_out, n_in)).copy()
        trans = np.zeros((batch, n_out))
        n_axis = np.array([grid[j] if j < n_out else 8 for j in range(n_in)], dtype=np.float64)
        k = rng.integers(-1, n_axis + 2, size=(n_points, n_in)).astype(np.float64)
        half = rng.integers(0, 2, size=(n_points, n_in)) * 0.5
        points = 2.0 * (k + half) / n_axis - 1.0
    else:  # one_cell
        centre = 0.3 * rng.uniform(-1, 1, size=(1, n_in))
        points = centre + 1e-4 * rng.normal(size=(n_points, n_in))
    pw = rng.normal(size=n_points) * np.exp2(rng.uniform(-6, 6, size=n_points))
    ow = 10 * rng.uniform(0.1, 1, size=batch)
    ow[0] = -ow[0]
    bg = np.arange(1, batch + 1, dtype=np.float64) * 0.37
    ds_dout = np.asfortranarray(rng.normal(size=grid + (batch,)))
    c = lambda a: np.ascontiguousarray(a, dtype=dtype)
    return SimpleNamespace(points=c(points), rotations=c(rot), translations=c(trans), backgrounds=c(bg), weights=c(ow),
                           point_weights=c(pw), grid=grid, ds_dout=np.asfortranarray(ds_dout, dtype=dtype),
                           batch=batch, n_in=n_in, n_out=n_out, n_points=n_points, kind=kind)


def write_case(path, d, b=0):
    """Pose `b` of `d` in the file layout of tests/ordered_host_check.cpp (fp32)."""
    grid = list(d.grid) + [1] * (4 - len(d.grid))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", d.n_in, d.n_out, d.n_points, 1, *grid))
        f.write(f32(d.rotations[b].T))  # column-major n_out x n_in
        f.write(f32(d.translations[b]))
        f.write(f32([d.backgrounds[b], d.weights[b]]))
        f.write(f32(d.points))
        f.write(f32(d.point_weights))
