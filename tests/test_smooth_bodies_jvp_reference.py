"""The numpy reference of the smooth rigid-body JVP (tests/smooth_bodies_jvp_reference.py) against the numpy forward
and pullback of tests/smooth_bodies_reference.py, in fp64.  CPU only.

The case is the base case of tests/test_smooth_bodies_jvp_gpu.py: tests/test_smooth_bodies_gpu.py::_case with
sizes = (300, 200, 0, 277) -- P = 777, K = 4 with one empty body, B = 3 -- and V = 2 tangents ~ N(0, 1), so that B, K
and V differ pairwise.  The adjoint bound and the central-difference step and bound are those of
tests/test_smooth_jvp_reference.py.  Every test also needs `dpr_amd.raster_smooth_bodies_jvp` to exist, so none of
them passes without the feature."""
import functools

import numpy as np
import pytest

import dpr_amd
from tests import smooth_bodies_jvp_reference as BJR
from tests import smooth_bodies_reference as SBR
from tests.test_smooth_bodies_gpu import _accepted, _case

PAIRS = [(2, 2), (3, 3), (3, 2)]
NAMES = ("points_dot", "rotation_dot", "translation_dot", "background_dot", "out_weight_dot", "point_weight_dot")
SIZES = (300, 200, 0, 277)
V = 2


def setup_module(_m):
    assert callable(dpr_amd.raster_smooth_bodies_jvp) and callable(dpr_amd.raster_smooth_bodies_jvp_)


def tangents(c, n_tangents, seed=0):
    """All six tangents ~ N(0, 1) of case `c` with a leading axis of `n_tangents` (rotation_dot is not symmetric)."""
    rng = np.random.default_rng(500 + seed)
    P, n_in = c["points"].shape
    B, K, n_out = c["B"], c["K"], len(c["grid"])
    return dict(points_dot=rng.normal(size=(n_tangents, P, n_in)),
                rotation_dot=rng.normal(size=(n_tangents, B, K, n_out, n_in)),
                translation_dot=rng.normal(size=(n_tangents, B, K, n_out)),
                background_dot=rng.normal(size=(n_tangents, B)), out_weight_dot=rng.normal(size=(n_tangents, B)),
                point_weight_dot=rng.normal(size=(n_tangents, P)))


def reference(c, n_tangents, tan, body=None, keep=None):
    """out_dot of case `c`; `body`: another body vector; `keep`: the points that take part."""
    body = c["body"] if body is None else body
    keep = slice(None) if keep is None else keep
    tan = {k: (v[:, keep] if k in ("points_dot", "point_weight_dot") else v) for k, v in tan.items()}
    return BJR.raster_smooth_bodies_jvp(c["grid"], c["points"][keep], body[keep], c["rot"], c["trans"], c["ow"],
                                        c["pw"][keep], V=n_tangents, **tan)


@functools.lru_cache(maxsize=None)
def _jv(n_in, n_out):
    c = _case(n_in, n_out, sizes=SIZES, seed=2)
    tan = tangents(c, V)
    return c, tan, reference(c, V, tan)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_adjoint_identity(n_in, n_out):
    """<J v, g> = sum_i <v_i, pullback_i(g)> for every tangent: J . v is the exact transpose of the pullback."""
    c, tan, jv = _jv(n_in, n_out)
    assert jv.shape == c["grid"] + (V, 3) and c["K"] == 4 and c["P"] == 777
    for v in range(V):
        lhs = float((jv[..., v, :] * c["g"]).sum())
        rhs = sum(float((tan[name][v] * grad).sum()) for name, grad in zip(NAMES, c["pb"]))
        bound = 1e-12 * np.linalg.norm(jv[..., v, :]) * np.linalg.norm(c["g"])
        print(f"({n_in},{n_out}) v={v}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert np.linalg.norm(jv[..., v, :]) > 0
        assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences(n_in, n_out):
    """Differences of the numpy forward along the joint tangent, step 1e-7: norm-wise within 1e-6."""
    c, tan, jv = _jv(n_in, n_out)
    h = 1e-7
    for v in range(V):
        def f(sign):
            return SBR.raster(c["grid"], c["points"] + sign * h * tan["points_dot"][v], c["body"],
                              c["rot"] + sign * h * tan["rotation_dot"][v],
                              c["trans"] + sign * h * tan["translation_dot"][v],
                              c["bg"] + sign * h * tan["background_dot"][v],
                              c["ow"] + sign * h * tan["out_weight_dot"][v],
                              c["pw"] + sign * h * tan["point_weight_dot"][v])
        fd = (f(+1) - f(-1)) / (2 * h)
        err = np.linalg.norm(fd - jv[..., v, :]) / np.linalg.norm(jv[..., v, :])
        print(f"({n_in},{n_out}) v={v}: central differences rel. error {err:.3e}")
        assert err <= 1e-6


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_an_omitted_tangent_is_a_zero_tangent(n_in, n_out):
    c, tan, jv = _jv(n_in, n_out)
    total = np.zeros_like(jv)
    for name in NAMES:
        alone = reference(c, V, {name: tan[name]})
        zeros = {m: (tan[m] if m == name else np.zeros_like(tan[m])) for m in NAMES}
        assert np.array_equal(alone, reference(c, V, zeros)), name
        assert np.any(alone), name
        total += alone
    # ... and J is linear in the tangents: the six parts add up to the joint derivative
    assert np.linalg.norm(total - jv) <= 1e-13 * np.linalg.norm(jv)
    assert not np.any(reference(c, V, {}))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_nan_tangents_of_dropped_points_change_nothing(n_in, n_out):
    """NaN in every tangent of the points no image accepts, and of points whose body lies outside [0, K)."""
    c, tan, jv = _jv(n_in, n_out)
    never = ~_accepted(c).any(axis=0)
    assert never.sum() > 10
    bad = dict(tan)
    for name in ("points_dot", "point_weight_dot"):
        bad[name] = tan[name].copy()
        bad[name][:, never] = np.nan
    assert np.array_equal(reference(c, V, bad), jv)
    # bodies out of range: the result is that of the call without those points
    body = np.array(c["body"])
    out = np.arange(100, 130)
    body[out] = np.resize([-1, c["K"], 2**31 - 1], 30)
    for name in ("points_dot", "point_weight_dot"):
        bad[name][:, out] = np.nan
    keep = np.setdiff1d(np.arange(c["P"]), out)
    got = reference(c, V, bad, body=body)
    assert np.isfinite(got).all() and np.array_equal(got, reference(c, V, tan, keep=keep))
