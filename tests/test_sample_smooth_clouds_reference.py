"""The numpy reference of smooth sampling at per-pose clouds (tests/sample_smooth_clouds_reference.py) against the
definition in include/dpr.h: central differences of its pullback in the image, the clouds and the poses, and the
adjoint identity with the smooth splat (tests/smooth_reference.py) of the per-pose clouds.  CPU only.  Every test also
needs `dpr_amd.sample_smooth_clouds` to exist, so none of them passes without the feature."""
import numpy as np
import pytest

import dpr_amd
from tests import sample_smooth_clouds_reference as SCR
from tests import sample_smooth_reference as SSR
from tests import smooth_reference as SR

PAIRS = [(2, 2), (3, 3), (3, 2)]
P, B = 10, 3


def setup_module(_m):
    assert callable(dpr_amd.sample_smooth_clouds) and callable(dpr_amd.sample_smooth_clouds_pullback_)


def _problem(n_in, n_out, seed):
    """8^N grid, B = 3 clouds of 10 points in +-1.1 (some in the halo bands, some with dropped cells)."""
    rng = np.random.default_rng(seed)
    grid = (8,) * n_out
    pts = rng.uniform(-1.1, 1.1, size=(B, P, n_in))
    q, _ = np.linalg.qr(rng.normal(size=(B, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :n_out, :])
    trans = rng.uniform(-0.1, 0.1, size=(B, n_out))
    image = rng.normal(size=grid + (B,))
    dv = rng.normal(size=(B, P))
    return grid, [image, pts, rot, trans], dv


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_rows_are_the_single_pose_reference(n_in, n_out):
    _grid, args, dv = _problem(n_in, n_out, seed=1)
    image, pts, rot, trans = args
    values = SCR.sample_smooth_clouds(*args)
    pb = SCR.sample_smooth_clouds_pullback(dv, *args)
    assert values.shape == (B, P) and pb[0].shape == image.shape and pb[1].shape == pts.shape
    assert pb[2].shape == rot.shape and pb[3].shape == trans.shape
    for b in range(B):
        one = [image[..., b:b + 1], pts[b], rot[b:b + 1], trans[b:b + 1]]
        assert np.array_equal(values[b], SSR.sample_smooth(*one)[:, 0])
        g = SSR.sample_smooth_pullback(dv[b][:, None], *one)
        assert np.array_equal(pb[0][..., b], g[0][..., 0]) and np.array_equal(pb[1][b], g[1])
        assert np.array_equal(pb[2][b], g[2][0]) and np.array_equal(pb[3][b], g[3][0])


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences_agree_with_the_pullback(n_in, n_out):
    """h = 1e-6, fp64, 8^N grid, 3 clouds of 10 points; within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_gpu.py)."""
    _grid, args, dv = _problem(n_in, n_out, seed=6)

    def loss(a):
        return float((SCR.sample_smooth_clouds(*a) * dv).sum())

    analytic = SCR.sample_smooth_clouds_pullback(dv, *args)
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
def test_adjoint_identity_with_the_smooth_splat_of_the_clouds(n_in, n_out):
    """Per pose, sum_v splat(pw)[v, b] * image[v, b] == sum_p pw[b, p] * values[b, p] to 1e-10 relative, and
    ds_dimage[..., b] is the smooth splat of cloud b with point_weight = dv[b] (background 0, out_weight 1)."""
    grid, args, dv = _problem(n_in, n_out, seed=8)
    image, pts, rot, trans = args
    values = SCR.sample_smooth_clouds(*args)
    d_img = SCR.sample_smooth_clouds_pullback(dv, *args)[0]
    for b in range(B):
        splat = SR.raster_smooth(grid, pts[b], rot[b:b + 1], trans[b:b + 1], point_weight=dv[b])[..., 0]
        lhs, rhs = float((splat * image[..., b]).sum()), float((dv[b] * values[b]).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (b, lhs, rhs)
        err = np.abs(d_img[..., b] - splat).max()
        assert err <= 1e-10 * np.abs(splat).max(), (b, err)
