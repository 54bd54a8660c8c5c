"""The numpy reference of the smooth splat (tests/smooth_reference.py) against the definition in include/dpr.h:
known answers, partition of unity, central differences of all six gradients, and the continuity of the gradient
across a cell boundary.  CPU only.  The module under test is importable from the package as well: every test also
needs `dpr_amd.raster_smooth` to exist, so none of them passes without the feature."""
import numpy as np
import pytest

import dpr_amd
from tests import smooth_reference as SR

PAIRS = [((7, 5), 2), ((6, 5, 4), 3), ((7, 5), 3)]  # (grid, n_in)


def setup_module(_m):
    assert callable(dpr_amd.raster_smooth) and callable(dpr_amd.raster_pullback_smooth_)


def _identity(n_out, n_in):
    return np.eye(n_out, n_in)[None]


def test_known_answer_centre_point():
    out = SR.raster_smooth((5, 5), np.zeros((1, 2)), _identity(2, 2), np.zeros((1, 2)))[..., 0]
    k = np.array([1 / 8, 3 / 4, 1 / 8])
    want = np.zeros((5, 5))
    want[1:4, 1:4] = np.outer(k, k)
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-15)


def test_known_answer_border_point():
    """(-1, 0): coord_x = 0, x-weights [1/2, 1/2, 0] with cell -1 dropped."""
    out = SR.raster_smooth((5, 5), np.array([[-1.0, 0.0]]), _identity(2, 2), np.zeros((1, 2)))[..., 0]
    want = np.zeros((5, 5))
    want[0, 1:4] = 0.5 * np.array([1 / 8, 3 / 4, 1 / 8])
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-15)
    assert abs(out.sum() - 0.5) < 1e-15


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_partition_of_unity_for_interior_points(grid, n_in):
    rng = np.random.default_rng(1)
    n_out = len(grid)
    # coord in [1.5, n - 1.5): every target cell is inside the grid
    lo = np.array([-1 + 3.0 / n for n in grid])
    pts = np.zeros((30, n_in))
    pts[:, :n_out] = rng.uniform(lo, -lo, size=(30, n_out))
    pw = rng.uniform(0.5, 2.0, 30)
    out = SR.raster_smooth(grid, pts, _identity(n_out, n_in), np.zeros((1, n_out)), point_weight=pw)
    assert abs(out.sum() - pw.sum()) < 1e-12
    assert out.min() >= 0


def _problem(grid, n_in, seed, P=40, B=2):
    rng = np.random.default_rng(seed)
    n_out = len(grid)
    pts = rng.uniform(-1.2, 1.2, size=(P, n_in))
    q, _ = np.linalg.qr(rng.normal(size=(B, 3, 3)))
    rot = np.ascontiguousarray(q[:, :n_out, :n_in]) if n_in == 3 else np.ascontiguousarray(q[:, :2, :2])
    trans = rng.uniform(-0.1, 0.1, size=(B, n_out))
    bg = rng.normal(size=B)
    ow = rng.uniform(0.5, 1.5, size=B)
    pw = rng.uniform(0.5, 1.5, size=P)
    g = rng.normal(size=tuple(grid) + (B,))
    return pts, rot, trans, bg, ow, pw, g


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_central_differences_agree_with_the_gradients(grid, n_in):
    pts, rot, trans, bg, ow, pw, g = _problem(grid, n_in, seed=3)
    args = [pts, rot, trans, bg, ow, pw]

    def loss(a):
        return float((SR.raster_smooth(grid, *a) * g).sum())

    # rejected points and dropped cells occur
    out = SR.raster_smooth(grid, pts, rot, trans)
    assert out.sum() < 2 * len(pts) - 1
    grads = SR.raster_pullback_smooth(g, pts, rot, trans, ow, pw)
    analytic = [grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]]
    scale = max(np.abs(a).max() for a in analytic)
    h = 1e-6
    for k, (x, ga) in enumerate(zip(args, analytic)):
        fd = np.zeros_like(x)
        it = np.nditer(x, flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            keep = x[i]
            x[i] = keep + h
            up = loss(args)
            x[i] = keep - h
            dn = loss(args)
            x[i] = keep
            fd[i] = (up - dn) / (2 * h)
        assert np.abs(fd - ga).max() <= 1e-6 * scale, (k, np.abs(fd - ga).max(), scale)


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_gradient_is_continuous_across_a_cell_boundary(grid, n_in):
    """Points 1e-9 either side of an integer coord (a change of the centre cell j0)."""
    rng = np.random.default_rng(5)
    n_out = len(grid)
    g = rng.normal(size=tuple(grid) + (1,))
    rot, trans = _identity(n_out, n_in), np.zeros((1, n_out))
    base = rng.uniform(-0.5, 0.5, size=(6, n_in))
    base[:, 0] = -1 + 2.0 * np.array([2, 3, 4, 2, 3, 4]) / grid[0]  # coord_0 = 2, 3, 4
    lo, hi = base.copy(), base.copy()
    lo[:, 0] -= 1e-9 * 2 / grid[0]
    hi[:, 0] += 1e-9 * 2 / grid[0]
    # the two sides do have different centre cells
    n0 = grid[0]
    assert np.all(np.floor((lo[:, 0] + 1) * n0 / 2) + 1 == np.floor((hi[:, 0] + 1) * n0 / 2))
    ga = SR.raster_pullback_smooth(g, lo, rot, trans)
    gb = SR.raster_pullback_smooth(g, hi, rot, trans)
    scale = max(np.abs(a).max() for a in ga)
    assert np.abs(ga[0] - gb[0]).max() < 1e-6 * scale
    assert np.abs(ga[5] - gb[5]).max() < 1e-6 * scale
