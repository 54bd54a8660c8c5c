"""The numpy reference of the smooth splat with channels (tests/smooth_channels_reference.py): its planes are the
single-channel smooth splat, its pullback is the transpose of the forward in every linear argument, and it agrees with
central differences in points and pose across a cell face.  CPU only, fp64.  Every test also needs
`dpr_amd.raster_smooth_channels` to exist, so none of them passes without the feature."""
import numpy as np
import pytest

import dpr_amd
from tests import smooth_channels_reference as SCR
from tests import smooth_reference as SR

PAIRS = [((7, 5), 2), ((6, 5, 4), 3), ((7, 5), 3)]  # (grid, n_in)
C = 3


def setup_module(_m):
    assert callable(dpr_amd.raster_smooth_channels) and callable(dpr_amd.raster_pullback_smooth_channels_)


def _problem(grid, n_in, seed, P=40, B=2):
    rng = np.random.default_rng(seed)
    n_out = len(grid)
    pts = rng.uniform(-1.2, 1.2, size=(P, n_in))
    q, _ = np.linalg.qr(rng.normal(size=(B, 3, 3)))
    rot = np.ascontiguousarray(q[:, :n_out, :n_in]) if n_in == 3 else np.ascontiguousarray(q[:, :2, :2])
    trans = rng.uniform(-0.1, 0.1, size=(B, n_out))
    bg = rng.normal(size=(B, C))
    ow = rng.uniform(0.5, 1.5, size=B)
    pw = rng.uniform(-1.0, 1.5, size=(P, C))
    g = rng.normal(size=tuple(grid) + (C, B))
    return pts, rot, trans, bg, ow, pw, g


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_planes_are_the_single_channel_smooth_splat(grid, n_in):
    pts, rot, trans, bg, ow, pw, _g = _problem(grid, n_in, seed=1)
    out = SCR.raster_smooth_channels(grid, pts, rot, trans, pw, bg, ow)
    assert out.shape == tuple(grid) + (C, 2)
    for c in range(C):
        want = SR.raster_smooth(grid, pts, rot, trans, bg[:, c], ow, pw[:, c])
        assert np.array_equal(out[..., c, :], want)
    # the defaults: background 0, out_weight 1
    out = SCR.raster_smooth_channels(grid, pts, rot, trans, pw)
    assert np.array_equal(out[..., 1, :], SR.raster_smooth(grid, pts, rot, trans, point_weight=pw[:, 1]))


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_pullback_is_the_transpose_of_the_forward(grid, n_in):
    """out is linear in background, in point_weight and, through out - background, in out_weight:
    <g, d out> = <pullback(g), d argument> for each."""
    pts, rot, trans, bg, ow, pw, g = _problem(grid, n_in, seed=2)
    rng = np.random.default_rng(9)
    _d_pts, _d_rot, _d_trans, d_bg, d_ow, d_pw = SCR.raster_pullback_smooth_channels(g, pts, rot, trans, pw, ow)
    zero = np.zeros_like(bg)
    # background: out(bg + v) - out(bg) = v broadcast over the cells
    v = rng.normal(size=bg.shape)
    lhs = (g * (SCR.raster_smooth_channels(grid, pts, rot, trans, pw, v, ow)
                - SCR.raster_smooth_channels(grid, pts, rot, trans, pw, zero, ow))).sum()
    assert abs(lhs - (d_bg * v).sum()) <= 1e-12 * max(1.0, abs(lhs))
    # point_weight
    v = rng.normal(size=pw.shape)
    lhs = (g * SCR.raster_smooth_channels(grid, pts, rot, trans, v, zero, ow)).sum()
    assert abs(lhs - (d_pw * v).sum()) <= 1e-12 * max(1.0, abs(lhs))
    # out_weight
    v = rng.normal(size=ow.shape)
    lhs = (g * SCR.raster_smooth_channels(grid, pts, rot, trans, pw, zero, v)).sum()
    assert abs(lhs - (d_ow * v).sum()) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("grid,n_in", PAIRS)
def test_central_differences_in_points_and_pose_across_a_cell_face(grid, n_in):
    """The bound of tests/test_smooth_reference.py: 1e-6 of the largest gradient entry.  Six of the points sit within
    1e-9 cells of a face of axis 0, so the two sides of their differences have different centre cells.  The operator
    is C1, not C2: across a face the second derivative jumps by J = O(n^2 |g| |pw|), and a central difference that
    straddles the face is off by about h J / 4 whatever the gradient code does.  With J of a few hundred here, the
    h = 1e-6 of that file would spend the whole bound on this term (3e-5 against 3e-5); h = 1e-7 leaves it a tenth of
    the bound, and the rounding of the loss (1e-14 / h = 1e-7) well below."""
    pts, rot, trans, bg, ow, pw, g = _problem(grid, n_in, seed=3)
    n_out = len(grid)
    rot[0] = np.eye(n_out, n_in)
    trans[0] = 0
    pts[:6, 0] = -1 + 2.0 * np.array([2, 3, 4, 2, 3, 4]) / grid[0] + 1e-9 * 2 / grid[0]
    pts[:6, 1:] = np.random.default_rng(4).uniform(-0.5, 0.5, size=(6, n_in - 1))
    n0 = grid[0]
    h = 1e-7
    assert np.all(np.floor((pts[:6, 0] - h + 1) * n0 / 2) + 1 == np.floor((pts[:6, 0] + h + 1) * n0 / 2))
    args = [pts, rot, trans]

    def loss(a):
        return float((SCR.raster_smooth_channels(grid, *a, pw, bg, ow) * g).sum())

    grads = SCR.raster_pullback_smooth_channels(g, pts, rot, trans, pw, ow)
    scale = max(np.abs(a).max() for a in grads)
    for k, (x, ga) in enumerate(zip(args, grads[:3])):
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
