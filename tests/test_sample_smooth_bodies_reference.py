"""The numpy reference of smooth sampling at the points of rigid bodies (tests/sample_smooth_bodies_reference.py)
against the definition in include/dpr.h (SMOOTH SAMPLING, RIGID BODIES): the adjoint identity against the splat of
rigid bodies, central differences of its pullback -- also across a cell face -- and the dropped bodies.  fp64, CPU
only.  Every test also needs `dpr_amd.sample_smooth_bodies` to exist, so none of them passes without the feature."""
import numpy as np
import pytest

import dpr_amd
from tests import sample_smooth_bodies_reference as ref
from tests import smooth_bodies_reference as SBR

PAIRS = [((7, 5), 2), ((6, 5, 4), 3), ((7, 5), 3)]  # (grid, n_in)


def setup_module(_m):
    assert callable(dpr_amd.sample_smooth_bodies) and callable(dpr_amd.sample_smooth_bodies_pullback_)


def _problem(grid, n_in, seed, P=40, B=3, K=3):
    rng = np.random.default_rng(seed)
    n_out = len(grid)
    pts = rng.uniform(-1.2, 1.2, size=(P, n_in))
    body = rng.integers(0, K, size=P)
    q, _ = np.linalg.qr(rng.normal(size=(B, K, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :, :n_out, :])
    trans = rng.uniform(-0.1, 0.1, size=(B, K, n_out))
    image = rng.normal(size=tuple(grid) + (B,))
    return pts, body, rot, trans, image


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_adjoint_identity_against_the_splat_of_rigid_bodies(grid, n_in):
    """sum_v raster(pw; bg 0, ow 1)[v, b] * image[v, b] = sum_p pw[p] * values[p, b] for every b, to 1e-12."""
    pts, body, rot, trans, image = _problem(grid, n_in, seed=1)
    pts *= 1.25  # +-1.5: beyond the one cell of margin of every axis
    pw = np.random.default_rng(2).uniform(0.5, 1.5, size=len(pts))
    out = SBR.raster(grid, pts, body, rot, trans, None, None, pw)
    values = ref.sample(image, pts, body, rot, trans)
    assert values.shape == (len(pts), 3)
    assert (values == 0).any() and (values != 0).any()  # rejected and accepted points
    for b in range(3):
        lhs = (out[..., b] * image[..., b]).sum()
        rhs = (pw * values[:, b]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (b, lhs, rhs)


def _central_differences(args, dv, h=1e-6):
    """Central differences of sum(values * dv) in image, points, rotation and translation (args[0], [1], [3], [4])."""
    def loss():
        return float((ref.sample(*args) * dv).sum())

    fds = []
    for x in (args[0], args[1], args[3], args[4]):
        fd = np.zeros_like(x)
        it = np.nditer(x, flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            keep = x[i]
            x[i] = keep + h
            up = loss()
            x[i] = keep - h
            dn = loss()
            x[i] = keep
            fd[i] = (up - dn) / (2 * h)
        fds.append(fd)
    return fds


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_central_differences_agree_with_the_pullback(n_in, n_out):
    """h = 1e-6, fp64, 8^N grid, 10 points of 2 bodies, B = 2; within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_reference.py)."""
    grid = (8,) * n_out
    pts, body, rot, trans, image = _problem(grid, n_in, seed=6, P=10, B=2, K=2)
    pts *= 1.1 / 1.2
    dv = np.random.default_rng(7).normal(size=(10, 2))
    args = [image, pts, body, rot, trans]
    analytic = ref.sample_pullback(dv, *args)
    assert analytic[2].shape == (2, 2, n_out, n_in) and analytic[3].shape == (2, 2, n_out)
    scale = max(np.abs(a).max() for a in analytic)
    for k, (fd, ga) in enumerate(zip(_central_differences(args, dv), analytic)):
        assert np.abs(fd - ga).max() <= 1e-6 * scale, (k, np.abs(fd - ga).max(), scale)


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_central_differences_hold_across_a_cell_face(n_in, n_out):
    """Two points 2.5e-8 cells from a face between two cells (coord = 3 and coord = 5 on an 8^N grid under the identity
    pose): the two sides of their differences sit in different centre cells, and the bound is the same, 1e-6 *
    max|gradient|.  The operator is C1, not C2: across a face the second derivative jumps by J = O(n^2 |image| |dv|),
    and a central difference that straddles the face is off by about h J / 4 whatever the gradient code does (the
    reasoning of tests/test_smooth_channels_reference.py).  At h = 1e-6 that term alone is 1e-5 here, twice the bound;
    h = 1e-7 leaves it a quarter of the bound and the rounding of the loss (1e-14 / h = 1e-7) well below."""
    grid = (8,) * n_out
    rng = np.random.default_rng(11)
    pts = rng.uniform(-0.5, 0.5, size=(4, n_in))
    h = 1e-7
    pts[0, 0] = -0.25 + 2.5e-8 * 2 / 8   # coord_0 = 3 + 2.5e-8
    pts[1, 1] = 0.25 - 2.5e-8 * 2 / 8    # coord_1 = 5 - 2.5e-8
    body = np.array([0, 1, 1, 0])
    rot = np.broadcast_to(np.eye(n_out, n_in), (1, 2, n_out, n_in)).copy()
    trans = np.zeros((1, 2, n_out))
    image = rng.normal(size=grid + (1,))
    dv = rng.normal(size=(4, 1))
    args = [image, pts, body, rot, trans]
    n = 8
    assert np.floor((pts[0, 0] + 1) * n / 2) == 3 and np.floor((pts[0, 0] - h + 1) * n / 2) == 2
    assert np.floor((pts[1, 1] + 1) * n / 2) == 4 and np.floor((pts[1, 1] + h + 1) * n / 2) == 5
    analytic = ref.sample_pullback(dv, *args)
    scale = max(np.abs(a).max() for a in analytic)
    for k, (fd, ga) in enumerate(zip(_central_differences(args, dv, h), analytic)):
        assert np.abs(fd - ga).max() <= 1e-6 * scale, (k, np.abs(fd - ga).max(), scale)


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_a_body_outside_the_range_gives_zeros(grid, n_in):
    pts, body, rot, trans, image = _problem(grid, n_in, seed=8)
    body = body.copy()
    out = np.array([0, 5, 11, 17])
    body[out] = [-1, 3, 2**31 - 1, -7]
    values = ref.sample(image, pts, body, rot, trans)
    assert (values[out] == 0).all() and (values != 0).any()
    dv = np.random.default_rng(9).normal(size=values.shape)
    d_img, d_pts, d_rot, d_trans = ref.sample_pullback(dv, image, pts, body, rot, trans)
    assert (d_pts[out] == 0).all() and (d_pts != 0).any()
    # ... and deposit nothing: the gradients are those of the cloud without them
    keep = np.setdiff1d(np.arange(len(pts)), out)
    rest = ref.sample_pullback(dv[keep], image, pts[keep], body[keep], rot, trans)
    np.testing.assert_array_equal(d_img, rest[0])
    np.testing.assert_array_equal(d_rot, rest[2])
    np.testing.assert_array_equal(d_trans, rest[3])


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_image_gradient_is_the_splat_of_the_value_gradients(grid, n_in):
    """ds_dimage[.., b] = raster_smooth_bodies of image b alone with point_weight = ds_dvalues[:, b]."""
    pts, body, rot, trans, image = _problem(grid, n_in, seed=12)
    dv = np.random.default_rng(13).normal(size=(len(pts), 3))
    d_img = ref.sample_pullback(dv, image, pts, body, rot, trans)[0]
    for b in range(3):
        want = SBR.raster(grid, pts, body, rot[b:b + 1], trans[b:b + 1], None, None, dv[:, b])[..., 0]
        np.testing.assert_allclose(d_img[..., b], want, rtol=0, atol=1e-13)
