"""The numpy reference of the smooth splat's forward-mode derivative (tests/smooth_jvp_reference.py) against the numpy
forward and pullback of tests/smooth_reference.py, in fp64.  CPU only.

The case is the one the GPU tests use (tests/test_smooth_gpu.py::_case): grids (37, 19, 21) / (150, 37) -- three
tiles and a partial last tile per axis -- 20 000 points in +-1.15 with the slab x_0 >= 0.7 empty, 2 000 points in
one cell and the corner-cell points; B = 3, K = 2, all six tangents ~ N(0, 1).  Every test also needs
`dpr_amd.raster_smooth_jvp` to exist, so none of them passes without the feature."""
import functools

import numpy as np
import pytest

import dpr_amd
from tests import smooth_jvp_reference as JR
from tests import smooth_reference as SR
from tests.test_smooth_gpu import _case

PAIRS = [(2, 2), (3, 3), (3, 2)]
NAMES = ("points_dot", "rotation_dot", "translation_dot", "background_dot", "out_weight_dot", "point_weight_dot")


def setup_module(_m):
    assert callable(dpr_amd.raster_smooth_jvp) and callable(dpr_amd.raster_smooth_jvp_)


def tangents(c, K, B, seed=0):
    """All six tangents ~ N(0, 1) for the first B poses of case `c` (rotation_dot is not symmetric)."""
    rng = np.random.default_rng(seed)
    P, n_in = c["points"].shape
    n_out = len(c["grid"])
    return dict(points_dot=rng.normal(size=(K, P, n_in)), rotation_dot=rng.normal(size=(K, B, n_out, n_in)),
                translation_dot=rng.normal(size=(K, B, n_out)), background_dot=rng.normal(size=(K, B)),
                out_weight_dot=rng.normal(size=(K, B)), point_weight_dot=rng.normal(size=(K, P)))


def reference(c, K, B, tan, dtype=np.float64):
    return JR.raster_smooth_jvp(c["grid"], c["points"], c["rot"][:B], c["trans"][:B], c["ow"][:B], c["pw"], K=K,
                                dtype=dtype, **tan)


@functools.lru_cache(maxsize=None)
def _jv(n_in, n_out):
    c = _case(n_in, n_out)
    tan = tangents(c, 2, 3)
    return c, tan, reference(c, 2, 3, tan)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_adjoint_identity(n_in, n_out):
    """<J v, g> = sum_i <v_i, pullback_i(g)> for every tangent k: J . v is the exact transpose of the pullback."""
    c, tan, jv = _jv(n_in, n_out)
    pb = c["pb"]  # of g = c["g"], with out_weight and point_weight
    for k in range(2):
        lhs = float((jv[..., k, :] * c["g"]).sum())
        rhs = sum(float((tan[name][k] * grad).sum()) for name, grad in zip(NAMES, pb))
        bound = 1e-12 * np.linalg.norm(jv[..., k, :]) * np.linalg.norm(c["g"])
        print(f"({n_in},{n_out}) k={k}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences(n_in, n_out):
    """Differences of the numpy forward along the joint tangent, step 1e-7: norm-wise within 1e-6."""
    c, tan, jv = _jv(n_in, n_out)
    h = 1e-7
    for k in range(2):
        def f(sign):
            return SR.raster_smooth(c["grid"], c["points"] + sign * h * tan["points_dot"][k],
                                    c["rot"] + sign * h * tan["rotation_dot"][k],
                                    c["trans"] + sign * h * tan["translation_dot"][k],
                                    c["bg"] + sign * h * tan["background_dot"][k],
                                    c["ow"] + sign * h * tan["out_weight_dot"][k],
                                    c["pw"] + sign * h * tan["point_weight_dot"][k])
        fd = (f(+1) - f(-1)) / (2 * h)
        err = np.linalg.norm(fd - jv[..., k, :]) / np.linalg.norm(jv[..., k, :])
        print(f"({n_in},{n_out}) k={k}: central differences rel. error {err:.3e}")
        assert err <= 1e-6


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_nan_tangents_of_rejected_points_change_nothing(n_in, n_out):
    c, tan, jv = _jv(n_in, n_out)
    rejected = np.ones(len(c["points"]), bool)
    for _b, idx, *_ in SR._terms(c["grid"], c["points"], c["rot"], c["trans"], np.float64):
        rejected[idx] = False
    assert rejected.sum() > 100  # points no pose accepts
    bad = dict(tan)
    bad["points_dot"] = tan["points_dot"].copy()
    bad["point_weight_dot"] = tan["point_weight_dot"].copy()
    bad["points_dot"][:, rejected] = np.nan
    bad["point_weight_dot"][:, rejected] = np.nan
    assert np.array_equal(reference(c, 2, 3, bad), jv)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_an_omitted_tangent_is_a_zero_tangent(n_in, n_out):
    c, tan, jv = _jv(n_in, n_out)
    total = np.zeros_like(jv)
    for name in NAMES:
        alone = reference(c, 2, 3, {name: tan[name]})
        zeros = {m: (tan[m] if m == name else np.zeros_like(tan[m])) for m in NAMES}
        assert np.array_equal(alone, reference(c, 2, 3, zeros)), name
        total += alone
    # ... and J is linear in the tangents: the six parts add up to the joint derivative
    assert np.linalg.norm(total - jv) <= 1e-13 * np.linalg.norm(jv)
    assert not np.any(reference(c, 2, 3, {}))


def test_magnitudes_are_the_same_loop_on_absolute_values():
    """`magnitudes=True` (the budget of tests/test_smooth_jvp_hard_gpu.py): for a single accepted point the sum of
    |deposit| plus |background_dot| is |out_dot - background_dot| + |background_dot| cell by cell and every cell of
    its 3^N stencil inside the grid counts once; for a cloud it bounds |out_dot| and counts every (point, cell)."""
    rng = np.random.default_rng(12)
    grid, K, B = (6, 5, 7), 2, 2
    rot, trans = np.stack([np.eye(3)] * B), np.zeros((B, 3))
    kw = dict(K=K, rotation_dot=rng.normal(size=(K, B, 3, 3)), translation_dot=rng.normal(size=(K, B, 3)),
              background_dot=rng.normal(size=(K, B)), out_weight_dot=rng.normal(size=(K, B)))
    one = np.array([[0.1, -0.95, 0.3]])  # (centre cell 0 on axis 1: a third of the stencil is dropped)
    tan = dict(points_dot=rng.normal(size=(K, 1, 3)), point_weight_dot=rng.normal(size=(K, 1)), **kw)
    out = JR.raster_smooth_jvp(grid, one, rot, trans, **tan)
    A, n = JR.raster_smooth_jvp(grid, one, rot, trans, magnitudes=True, **tan)
    bgd = kw["background_dot"]
    assert A.shape == out.shape and n.shape == grid + (B,) and n.dtype == np.int64
    np.testing.assert_allclose(A, np.abs(out - bgd) + np.abs(bgd), rtol=1e-14, atol=0)
    assert np.all(n.sum(axis=(0, 1, 2)) == 18) and n.max() == 1
    pts = rng.uniform(-1.2, 1.2, size=(200, 3))
    tan = dict(points_dot=rng.normal(size=(K, 200, 3)), point_weight_dot=rng.normal(size=(K, 200)), **kw)
    out = JR.raster_smooth_jvp(grid, pts, rot, trans, **tan)
    A, n = JR.raster_smooth_jvp(grid, pts, rot, trans, magnitudes=True, **tan)
    empty = np.broadcast_to((n == 0)[..., None, :], A.shape)
    assert np.all(A >= np.abs(out) * (1 - 1e-12)) and np.all(A[empty] == np.abs(np.broadcast_to(bgd, A.shape))[empty])
    _b, _idx, j0, _w, _dw = next(iter(SR._terms(grid, pts, rot[:1], trans[:1], np.float64)))
    per_axis = [((j0[:, d, None] + np.arange(-1, 2) >= 0) & (j0[:, d, None] + np.arange(-1, 2) < grid[d])).sum(axis=1)
                for d in range(3)]
    assert n[..., 0].sum() == int((per_axis[0] * per_axis[1] * per_axis[2]).sum()) > 0
