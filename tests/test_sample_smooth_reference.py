"""The numpy reference of smooth sampling (tests/sample_smooth_reference.py) against the definition in include/dpr.h:
the three identities, a known answer and central differences of its pullback.  CPU only.  Every test also needs
`dpr_amd.sample_smooth` to exist, so none of them passes without the feature."""
import numpy as np
import pytest

import dpr_amd
from tests import sample_smooth_reference as SSR
from tests import smooth_reference as SR

PAIRS = [((7, 5), 2), ((6, 5, 4), 3), ((7, 5), 3)]  # (grid, n_in)


def setup_module(_m):
    assert callable(dpr_amd.sample_smooth) and callable(dpr_amd.sample_smooth_pullback_)


def _problem(grid, n_in, seed, P=40, B=3):
    rng = np.random.default_rng(seed)
    n_out = len(grid)
    pts = rng.uniform(-1.2, 1.2, size=(P, n_in))
    q, _ = np.linalg.qr(rng.normal(size=(B, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :n_out, :])
    trans = rng.uniform(-0.1, 0.1, size=(B, n_out))
    image = rng.normal(size=tuple(grid) + (B,))
    return pts, rot, trans, image


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_adjoint_identity_against_the_smooth_splat(grid, n_in):
    """sum_v (raster_smooth(pw) - background) * image = out_weight * sum_p pw * values, per pose (B = 3)."""
    pts, rot, trans, image = _problem(grid, n_in, seed=1)
    pts *= 1.25  # +-1.5: beyond the one cell of margin of every axis
    rng = np.random.default_rng(2)
    bg, ow, pw = rng.normal(size=3), rng.uniform(0.5, 1.5, size=3), rng.uniform(0.5, 1.5, size=len(pts))
    out = SR.raster_smooth(grid, pts, rot, trans, bg, ow, pw)
    values = SSR.sample_smooth(image, pts, rot, trans)
    assert (values == 0).any() and (values != 0).any()  # rejected and accepted points
    for b in range(3):
        lhs = ((out[..., b] - bg[b]) * image[..., b]).sum()
        rhs = ow[b] * (pw * values[:, b]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (b, lhs, rhs)


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_single_pose_values_are_the_splat_pullbacks_point_weight_gradient(grid, n_in):
    pts, rot, trans, image = _problem(grid, n_in, seed=3, B=1)
    values = SSR.sample_smooth(image, pts, rot, trans)
    d_pw = SR.raster_pullback_smooth(image, pts, rot, trans)[5]
    np.testing.assert_allclose(values[:, 0], d_pw, rtol=0, atol=1e-12 * np.abs(d_pw).max())


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_constant_image_samples_to_the_constant_inside(grid, n_in):
    """Points at least 1.5 cells inside the grid (coord in [1.5, n - 1.5)): all 3^N cells exist, the weights sum
    to 1."""
    rng = np.random.default_rng(4)
    n_out = len(grid)
    lo = np.array([-1 + 3.0 / n for n in grid])
    pts = np.zeros((30, n_in))
    pts[:, :n_out] = rng.uniform(lo, -lo, size=(30, n_out))
    image = np.full(tuple(grid) + (1,), 2.75)
    values = SSR.sample_smooth(image, pts, np.eye(n_out, n_in)[None], np.zeros((1, n_out)))
    np.testing.assert_allclose(values, 2.75, rtol=0, atol=1e-14)
    # ... and not at a point half a cell from the border, where a column of cells is dropped
    edge = np.zeros((1, n_in))
    edge[0, 0] = -1 + 1.0 / grid[0]
    v = SSR.sample_smooth(image, edge, np.eye(n_out, n_in)[None], np.zeros((1, n_out)))
    assert abs(v[0, 0] - 2.75 * 7 / 8) < 1e-14


def test_known_answer_centre_point():
    """A point at the centre of cell (2, 2) of a 5 x 5 image: sum k_i k_j image[1 + i, 1 + j], k = (1/8, 3/4, 1/8)."""
    image = np.random.default_rng(5).normal(size=(5, 5, 1))
    values = SSR.sample_smooth(image, np.zeros((1, 2)), np.eye(2)[None], np.zeros((1, 2)))
    k = np.array([1 / 8, 3 / 4, 1 / 8])
    want = sum(k[i] * k[j] * image[1 + i, 1 + j, 0] for i in range(3) for j in range(3))
    assert abs(values[0, 0] - want) <= 1e-15


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_central_differences_agree_with_the_pullback(n_in, n_out):
    """h = 1e-6, fp64, 8^N grid, 10 points, B = 2; within 1e-6 * max|gradient| (the bound of
    tests/test_smooth_reference.py)."""
    grid = (8,) * n_out
    pts, rot, trans, image = _problem(grid, n_in, seed=6, P=10, B=2)
    pts *= 1.1 / 1.2
    dv = np.random.default_rng(7).normal(size=(10, 2))
    args = [image, pts, rot, trans]

    def loss(a):
        return float((SSR.sample_smooth(*a) * dv).sum())

    analytic = SSR.sample_smooth_pullback(dv, *args)
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
def test_image_gradient_is_the_splat_of_the_value_gradients(grid, n_in):
    pts, rot, trans, image = _problem(grid, n_in, seed=8)
    dv = np.random.default_rng(9).normal(size=(len(pts), 3))
    d_img = SSR.sample_smooth_pullback(dv, image, pts, rot, trans)[0]
    for b in range(3):
        want = SR.raster_smooth(grid, pts, rot[b:b + 1], trans[b:b + 1], point_weight=dv[:, b])[..., 0]
        np.testing.assert_allclose(d_img[..., b], want, rtol=0, atol=1e-13)
