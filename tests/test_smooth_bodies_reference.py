"""The reference composition of tests/smooth_bodies_reference.py against what it is made of (tests/smooth_reference.py)
and against central differences.  CPU only."""
import numpy as np
import pytest

from tests import smooth_bodies_reference as ref
from tests import smooth_reference as SR

PAIRS = [(2, 2), (3, 3), (3, 2)]
NAMES = ("points", "rotation", "translation", "background", "out_weight", "point_weight")


def _poses(rng, n, n_in, n_out):
    q, _ = np.linalg.qr(rng.normal(size=(n, n_in, n_in)))
    return np.ascontiguousarray(q[:, :n_out, :]), rng.uniform(-0.08, 0.08, size=(n, n_out))


def _problem(n_in, n_out, B, K, P, grid, seed):
    rng = np.random.default_rng(seed)
    rot, trans = _poses(rng, B * K, n_in, n_out)
    return dict(grid=tuple(grid), points=rng.uniform(-1.15, 1.15, size=(P, n_in)), body=rng.integers(0, K, size=P),
                rot=rot.reshape(B, K, n_out, n_in), trans=trans.reshape(B, K, n_out), bg=rng.normal(size=B),
                ow=rng.uniform(0.5, 1.5, size=B), pw=rng.uniform(0.5, 1.5, size=P),
                ds=rng.normal(size=tuple(grid) + (B,)))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_for_one_body_the_reference_is_the_smooth_reference(n_in, n_out, npdt):
    c = _problem(n_in, n_out, B=3, K=1, P=200, grid=(9, 7, 5)[:n_out], seed=n_in + n_out)
    body = np.zeros(200, dtype=np.int64)
    want = SR.raster_smooth(c["grid"], c["points"], c["rot"][:, 0], c["trans"][:, 0], None, c["ow"], c["pw"],
                            dtype=npdt)
    got = ref.raster(c["grid"], c["points"], body, c["rot"], c["trans"], None, c["ow"], c["pw"], dtype=npdt)
    assert got.dtype == npdt and np.array_equal(got, want)
    # the background is added behind the sum, the smooth reference starts from it: one rounding apart
    want = SR.raster_smooth(c["grid"], c["points"], c["rot"][:, 0], c["trans"][:, 0], c["bg"], c["ow"], c["pw"],
                            dtype=npdt)
    got = ref.raster(c["grid"], c["points"], body, c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], dtype=npdt)
    assert np.abs(got - want).max() <= 8 * np.finfo(npdt).eps * np.abs(want).max()
    r = SR.raster_pullback_smooth(c["ds"], c["points"], c["rot"][:, 0], c["trans"][:, 0], c["ow"], c["pw"],
                                  dtype=npdt)
    g = ref.raster_pullback(c["ds"], c["points"], body, c["rot"], c["trans"], c["ow"], c["pw"], dtype=npdt)
    assert g[1].shape == (3, 1, n_out, n_in) and g[2].shape == (3, 1, n_out)
    for i in (0, 3, 4, 5):
        assert np.array_equal(g[i], r[i]), NAMES[i]
    assert np.array_equal(g[1][:, 0], r[1]) and np.array_equal(g[2][:, 0], r[2])


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_relabelling_the_bodies_with_the_poses_permuted_leaves_out_unchanged(n_in, n_out):
    K = 4
    c = _problem(n_in, n_out, B=2, K=K, P=300, grid=(9, 7, 5)[:n_out], seed=20 + n_in + n_out)
    c["body"][:5] = (-1, K, 2**31 - 1, -5, 9)  # outside [0, K): in no subset, under either labelling
    sigma = np.array([2, 0, 3, 1])             # body k becomes body sigma[k]
    inside = (c["body"] >= 0) & (c["body"] < K)
    body2 = np.where(inside, sigma[np.clip(c["body"], 0, K - 1)], c["body"])
    rot2, trans2 = np.empty_like(c["rot"]), np.empty_like(c["trans"])
    rot2[:, sigma], trans2[:, sigma] = c["rot"], c["trans"]
    a = ref.raster(c["grid"], c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    b = ref.raster(c["grid"], c["points"], body2, rot2, trans2, c["bg"], c["ow"], c["pw"])
    # (the subsets are added in another order: rounding level)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    ga = ref.raster_pullback(c["ds"], c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"])
    gb = ref.raster_pullback(c["ds"], c["points"], body2, rot2, trans2, c["ow"], c["pw"])
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[5], gb[5]) and np.array_equal(ga[3], gb[3])
    assert np.array_equal(ga[1], gb[1][:, sigma]) and np.array_equal(ga[2], gb[2][:, sigma])
    assert np.abs(ga[4] - gb[4]).max() <= 1e-12 * np.abs(ga[4]).max()
    assert not ga[0][:5].any() and not ga[5][:5].any()
    # a cloud without accepted points: the background, zero gradients, the grid sum
    none = np.full(300, 7)
    out = ref.raster(c["grid"], c["points"], none, c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    assert np.array_equal(out, np.broadcast_to(c["bg"], out.shape))
    g = ref.raster_pullback(c["ds"], c["points"], none, c["rot"], c["trans"], c["ow"], c["pw"])
    assert not any(g[i].any() for i in (0, 1, 2, 4, 5))
    assert np.allclose(g[3], c["ds"].reshape(-1, 2).sum(axis=0), rtol=1e-13)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_the_pullback_is_the_derivative_of_the_forward(n_in, n_out):
    """fp64 central differences, h = 1e-6, of sum(out * g) in all six arguments on an 8^N grid with 2 images, 3 bodies
    and 12 points: within 1e-6 * max|gradient|, the bound of tests/test_smooth_gpu.py -- the composition is a sum of
    cases already under that bound."""
    c = _problem(n_in, n_out, B=2, K=3, P=12, grid=(8,) * n_out, seed=40 + n_in + n_out)
    c["body"] = np.arange(12) % 3
    xs = [c["points"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"]]
    loss = lambda: float((ref.raster(c["grid"], xs[0], c["body"], *xs[1:]) * c["ds"]).sum())
    grads = ref.raster_pullback(c["ds"], xs[0], c["body"], xs[1], xs[2], xs[4], xs[5])
    scale = max(np.abs(g).max() for g in grads)
    assert scale > 0
    h = 1e-6
    for name, x, ga in zip(NAMES, xs, grads):
        assert ga.shape == x.shape, name
        flat = x.reshape(-1)  # (a view: the arrays are contiguous)
        fd = np.zeros(flat.size)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = loss()
            flat[i] = keep - h
            dn = loss()
            flat[i] = keep
            fd[i] = (up - dn) / (2 * h)
        err = np.abs(fd.reshape(ga.shape) - ga).max()
        assert err <= 1e-6 * scale, (name, err, scale)
