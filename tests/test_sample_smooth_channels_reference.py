"""The numpy reference of smooth sampling of C-channel images (tests/sample_smooth_channels_reference.py) against the
definition in include/dpr.h: central differences of its pullback, and the transpose identity with the smooth channel
splat.  CPU only.  Every test also needs `dpr_amd.sample_smooth_channels` to exist, so none of them passes without the
feature."""
import numpy as np
import pytest

import dpr_amd
from tests import sample_smooth_channels_reference as SCR
from tests import sample_smooth_reference as SSR
from tests import smooth_channels_reference as CR

PAIRS = [(2, 2), (3, 3), (3, 2)]
P, B, C = 10, 2, 3


def setup_module(_m):
    assert callable(dpr_amd.sample_smooth_channels) and callable(dpr_amd.sample_smooth_channels_pullback_)


def _problem(n_in, n_out, seed):
    """8^N grid, 10 points in +-1.1 (some in the halo bands, some with dropped cells), B = 2, C = 3."""
    rng = np.random.default_rng(seed)
    grid = (8,) * n_out
    pts = rng.uniform(-1.1, 1.1, size=(P, n_in))
    q, _ = np.linalg.qr(rng.normal(size=(B, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :n_out, :])
    trans = rng.uniform(-0.1, 0.1, size=(B, n_out))
    image = rng.normal(size=grid + (C, B))
    dv = rng.normal(size=(P, C, B))
    return grid, [image, pts, rot, trans], dv


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_planes_are_the_single_channel_reference(n_in, n_out):
    _grid, args, dv = _problem(n_in, n_out, seed=1)
    values = SCR.sample_smooth_channels(*args)
    assert values.shape == (P, C, B)
    pb = SCR.sample_smooth_channels_pullback(dv, *args)
    assert pb[0].shape == args[0].shape
    total = [0, 0, 0]
    for c in range(C):
        assert np.array_equal(values[:, c, :], SSR.sample_smooth(args[0][..., c, :], *args[1:]))
        one = SSR.sample_smooth_pullback(dv[:, c, :], args[0][..., c, :], *args[1:])
        assert np.array_equal(pb[0][..., c, :], one[0])
        total = [t + g for t, g in zip(total, one[1:])]
    for got, want in zip(pb[1:], total):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences_agree_with_the_pullback(n_in, n_out):
    """h = 1e-6, fp64, 8^N grid, 10 points, B = 2, C = 3; within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_gpu.py)."""
    _grid, args, dv = _problem(n_in, n_out, seed=6)

    def loss(a):
        return float((SCR.sample_smooth_channels(*a) * dv).sum())

    analytic = SCR.sample_smooth_channels_pullback(dv, *args)
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


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_transpose_identity_with_the_smooth_channel_splat(n_in, n_out):
    """<values, dv> == <image, ds_dimage> to 1e-10 relative, and ds_dimage[..., b] is the smooth channel splat of
    pose b with point_weight = dv[..., b] (background 0, out_weight 1)."""
    grid, args, dv = _problem(n_in, n_out, seed=8)
    image, pts, rot, trans = args
    values = SCR.sample_smooth_channels(*args)
    d_img = SCR.sample_smooth_channels_pullback(dv, *args)[0]
    lhs, rhs = float((values * dv).sum()), float((image * d_img).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    for b in range(B):
        want = CR.raster_smooth_channels(grid, pts, rot[b:b + 1], trans[b:b + 1], dv[..., b])[..., 0]
        err = np.abs(d_img[..., b] - want).max()
        assert err <= 1e-10 * np.abs(want).max(), (b, err)
