"""Smooth sampling of C-channel images on the GPU (dpr_amd.sample_smooth_channels / sample_smooth_channels_pullback_ /
sample_smooth_channels_ad) against the numpy reference tests/sample_smooth_channels_reference.py evaluated in fp64.
The interpolant is C1, so a different fp32 cell choice changes nothing at first order and no same-precision oracle is
needed.  Tolerances: the project's norm-wise ones (tests/test_parity_gpu.py: fp64 1e-10; fp32 5e-5 "out" for
ds_dimage, 1e-4 "points" for values and ds_dpoints, 1e-3 "pose" for ds_drotation and ds_dtranslation), with the kinds
of tests/test_sample_smooth_gpu.py.

The grids (150, 37) and (37, 19, 21) are 3 x 3 and 3 x 3 x 3 ragged tiles of the tiled path.  The cloud has about 3000
points: most inside, some in the halo bands coord in [-1, 0) and [n, n + 1) of pose 0 (the identity), some rejected.
One reference for C = 16 and B = 3 per pair serves every C and both batch forms: the operator is plane by plane, and
the geometric gradients are sums of per-plane ones."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests import sample_smooth_channels_reference as SCR
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol
from tests.test_smooth_gpu import _poses

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (150, 37), 3: (37, 19, 21)}
FIELDS = ("image", "points", "rotation", "translation")
KINDS = ("out", "points", "pose", "pose")
CMAX, NB = 16, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out):
    """Inputs (fp64 numpy) for C = 16, B = 3 and the fp64 per-plane reference results for B = 3 and B = 1, computed
    once and shared; never modified."""
    rng = np.random.default_rng(4000 + 10 * n_in + n_out)
    grid = GRIDS[n_out]
    n = np.asarray(grid, dtype=np.float64)
    uni = rng.uniform(-1.15, 1.15, size=(2800, n_in))
    halo = rng.uniform(-0.9, 0.9, size=(120, n_in))  # one axis in the halo band, below or above the grid
    for k in range(len(halo)):
        d = k % n_out
        off = 1 + rng.uniform(0.05, 0.95) * 2 / n[d]
        halo[k, d] = off if k % 2 else -off
    out = rng.uniform(-0.9, 0.9, size=(80, n_in))  # rejected by every pose
    out[:, 0] = np.where(np.arange(80) % 2 == 0, 1.4, -1.4)
    pts = np.concatenate([uni, halo, out])
    rng.shuffle(pts)
    rot, trans = _poses(rng, NB, n_in, n_out)
    image = rng.normal(size=grid + (CMAX, NB))
    dv = rng.normal(size=(len(pts), CMAX, NB))
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, image=image, dv=dv,
             values=SCR.sample_smooth_channels(image, pts, rot, trans))
    c["parts", NB] = SCR.pullback_parts(dv, image, pts, rot, trans)
    c["parts", 1] = SCR.pullback_parts(dv[..., :1], image[..., :1], pts, rot[:1], trans[:1])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _ref_pullback(c, C, B):
    return SCR.combine(c["parts", B][:C])


def _values_to_dev(a, dev):
    """numpy (P, C, B) -> the (P, C, B) view of a contiguous (B, P, C) device tensor."""
    return T(np.ascontiguousarray(a.transpose(2, 0, 1)), dev).permute(1, 2, 0)


def _dev_args(c, dev, npdt, C, B):
    return [grid_to_dev(c["image"][..., :C, :B].astype(npdt), dev), T(c["points"].astype(npdt), dev),
            T(c["rot"][:B].astype(npdt), dev), T(c["trans"][:B].astype(npdt), dev)]


def _single(args):
    """The single-pose form of batched device arguments with B = 1."""
    img, pts, rot, trans = args
    return [dpr_amd.to_grid_layout(img[..., 0]), pts, rot[0], trans[0]]


def _check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_matches_the_reference(dev, C, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    P = len(c["points"])
    # pose 0 (the identity) reaches the branches the cloud is built for
    n = np.asarray(c["grid"], dtype=np.float64)
    coord = (c["points"][:, :n_out] + 1) * n / 2
    rejected = np.any((coord < -1 - 1e-3) | (coord > n + 1 + 1e-3), axis=1)
    accepted = np.all((coord >= -1) & (coord < n + 1), axis=1)
    in_halo = accepted & np.any((coord < 0) | (coord >= n), axis=1)
    assert rejected.sum() > 100 and in_halo.sum() > 100 and accepted.sum() > 2000
    assert np.all(c["values"][rejected, :, 0] == 0) and np.all(c["values"][in_halo, :, 0] != 0)
    rej = torch.as_tensor(rejected, device=dev)
    args = _dev_args(c, dev, npdt, C, NB)
    v = dpr_amd.sample_smooth_channels(*args)
    assert v.shape == (P, C, NB) and v.dtype == tdt and v.permute(2, 0, 1).is_contiguous()
    assert_close(v, c["values"][:, :C].astype(npdt), tol(npdt, "points"), f"C={C} B={NB}")
    assert bool((v[rej][..., 0] == 0).all())
    # the single-pose form: (P, C)
    v1 = dpr_amd.sample_smooth_channels(*_single(_dev_args(c, dev, npdt, C, 1)), algo="atomic")
    assert v1.shape == (P, C) and v1.is_contiguous()
    assert_close(v1, c["values"][:, :C, 0].astype(npdt), tol(npdt, "points"), f"C={C} single pose")
    assert bool((v1[rej] == 0).all())


@pytest.mark.parametrize("C", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_every_plane_has_the_bits_of_sample_smooth(dev, C, npdt, tdt, n_in, n_out):
    """values[:, c, b] == sample_smooth_ of plane (c, b): no atomics, one order of contraction."""
    c = _case(n_in, n_out)
    P = len(c["points"])
    img, pts, rot, trans = _dev_args(c, dev, npdt, C, NB)
    v = dpr_amd.sample_smooth_channels(img, pts, rot, trans)
    for ch in range(C):
        plane = dpr_amd.to_grid_layout(img[..., ch, :])
        want = dpr_amd.sample_smooth_(torch.empty((NB, P), dtype=tdt, device=dev).t(), plane, pts, rot, trans)
        assert torch.equal(v[:, ch, :], want), f"C={C}: channel {ch}"
    if C % 4 == 0:  # fp32 stores groups of four as 16 bytes only into a 16-byte aligned `values`: one element off
        off = torch.empty((NB * P * C + 1,), dtype=tdt, device=dev)[1:].view(NB, P, C).permute(1, 2, 0)
        assert off.data_ptr() % 16 != 0
        assert torch.equal(dpr_amd.sample_smooth_channels_(off, img, pts, rot, trans), v)
    if C == 1:  # ... and as a whole, in the single-pose form too
        assert torch.equal(v[:, 0, :], dpr_amd.sample_smooth(dpr_amd.to_grid_layout(img[..., 0, :]), pts, rot, trans))
        s = _single(_dev_args(c, dev, npdt, 1, 1))
        assert torch.equal(dpr_amd.sample_smooth_channels(*s)[:, 0],
                           dpr_amd.sample_smooth(dpr_amd.to_grid_layout(s[0][..., 0]), *s[1:]))


# ------------------------------------------------------------------ pullback
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("C", [1, 3, 5, 16])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_matches_the_reference(dev, algo, C, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    dv = _values_to_dev(c["dv"][:, :C].astype(npdt), dev)
    pb = dpr_amd.sample_smooth_channels_pullback_(dv, *_dev_args(c, dev, npdt, C, NB), algo=algo)
    assert pb.image.shape == c["grid"] + (C, NB) and pb.points.dtype == tdt
    assert pb.image.permute(*reversed(range(pb.image.ndim))).is_contiguous()
    assert pb.rotation.shape == (NB, n_out, n_in) and pb.translation.shape == (NB, n_out)
    _check_pullback(pb, _ref_pullback(c, C, NB), npdt, f"{algo} C={C} B={NB} ")
    # single pose: unbatched results
    p1 = dpr_amd.sample_smooth_channels_pullback_(T(c["dv"][:, :C, 0].astype(npdt), dev),
                                                  *_single(_dev_args(c, dev, npdt, C, 1)), algo=algo)
    assert p1.image.shape == c["grid"] + (C,) and p1.rotation.shape == (n_out, n_in)
    assert p1.translation.shape == (n_out,)
    ref = _ref_pullback(c, C, 1)
    _check_pullback(p1, (ref[0][..., 0], ref[1], ref[2][0], ref[3][0]), npdt, f"{algo} C={C} single pose ")


@pytest.mark.parametrize("C", [1, 3, 5, 16])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_image_planes_are_the_tiled_smooth_channel_forward(dev, C, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    img, pts, rot, trans = _dev_args(c, dev, npdt, C, NB)
    dv = _values_to_dev(c["dv"][:, :C].astype(npdt), dev)
    pb = dpr_amd.sample_smooth_channels_pullback_(dv, img, pts, rot, trans, need=("image",), algo="tiled")
    assert pb.points is None and pb.rotation is None and pb.translation is None
    for b in range(NB):
        assert dv[..., b].is_contiguous()  # (a point_weight as it stands)
        want = dpr_amd.raster_smooth_channels_(dpr_amd.empty_channel_grid(c["grid"], C, None, tdt, dev), pts, rot[b],
                                               trans[b], point_weight=dv[..., b], algo="tiled")
        assert_close(pb.image[..., b], want.cpu().numpy(), tol(npdt, "out"), f"C={C}: pose {b}")


# ------------------------------------------------------------------ pose slicing
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_many_poses_of_a_small_cloud(dev, npdt, tdt, n_in, n_out):
    """B = 70, P = 300 on an 8^N grid: two blocks of points, so the launch cuts the poses into slices and ds_dpoints
    is added atomically.  C = 5: a group of four planes and one more."""
    rng = np.random.default_rng(7)
    B, P, C, grid = 70, 300, 5, (8,) * n_out
    pts = rng.uniform(-1.15, 1.15, size=(P, n_in))
    rot, trans = _poses(rng, B, n_in, n_out)
    image, dv = rng.normal(size=grid + (C, B)), rng.normal(size=(P, C, B))
    a = [grid_to_dev(image.astype(npdt), dev)] + [T(x.astype(npdt), dev) for x in (pts, rot, trans)]
    v = dpr_amd.sample_smooth_channels(*a)
    assert_close(v, SCR.sample_smooth_channels(image, pts, rot, trans).astype(npdt), tol(npdt, "points"), "B=70 values")
    ref = SCR.sample_smooth_channels_pullback(dv, image, pts, rot, trans)
    for algo in ("atomic", "tiled"):
        pb = dpr_amd.sample_smooth_channels_pullback_(_values_to_dev(dv.astype(npdt), dev), *a, algo=algo)
        _check_pullback(pb, ref, npdt, f"B=70 {algo} ")


# ------------------------------------------------------------------ derivative tests on the device
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, n_in, n_out):
    """sample_smooth_channels_ad in fp64 on an 8^N grid with 10 points, B = 2 and C = 3: central differences with
    h = 1e-6 of sum(values * dv) in image, points, rotation and translation, within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_gpu.py)."""
    rng = np.random.default_rng(11)
    B, P, C, grid = 2, 10, 3, (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    vals = [rng.normal(size=grid + (C, B)), rng.uniform(-1.1, 1.1, size=(P, n_in)), rot, trans]
    dv = T(rng.normal(size=(P, C, B)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    (dpr_amd.sample_smooth_channels_ad(*xs) * dv).sum().backward()
    grads = [x.grad.cpu().numpy() for x in xs]
    assert all(g.shape == v.shape for g, v in zip(grads, vals))
    scale = max(np.abs(a).max() for a in grads)
    h = 1e-6
    with torch.no_grad():
        for k, (x, ga) in enumerate(zip(xs, grads)):
            flat = x.view(-1)
            fd = np.zeros(flat.numel())
            for i in range(flat.numel()):
                keep = float(flat[i])
                flat[i] = keep + h
                up = float((dpr_amd.sample_smooth_channels(*xs) * dv).sum())
                flat[i] = keep - h
                dn = float((dpr_amd.sample_smooth_channels(*xs) * dv).sum())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (FIELDS[k], err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_values_and_gradients_are_continuous_across_a_cell_boundary(dev, n_in, n_out):
    """Points 1e-9 of a cell either side of an integer coord (fp64): values and all four gradients differ by less
    than 1e-6 * max|gradient|, and agree with the reference on both sides."""
    rng = np.random.default_rng(5)
    grid, C = (8,) * n_out, 3
    image = rng.normal(size=grid + (C, 1))
    rot, trans = np.eye(n_out, n_in)[None], np.zeros((1, n_out))
    base = rng.uniform(-0.5, 0.5, size=(6, n_in))
    base[:, 0] = -1 + 2.0 * np.array([2, 3, 4, 5, 6, 3]) / grid[0]
    lo, hi = base.copy(), base.copy()
    lo[:, 0] -= 1e-9 * 2 / grid[0]
    hi[:, 0] += 1e-9 * 2 / grid[0]
    assert np.all(np.floor((lo[:, 0] + 1) * 4) + 1 == np.floor((hi[:, 0] + 1) * 4))
    dv = rng.normal(size=(6, C, 1))
    img_d, dv_d = grid_to_dev(image, dev), _values_to_dev(dv, dev)
    res = []
    for p in (lo, hi):
        a = (T(p, dev), T(rot, dev), T(trans, dev))
        v = dpr_amd.sample_smooth_channels(img_d, *a)
        pb = dpr_amd.sample_smooth_channels_pullback_(dv_d, img_d, *a)
        assert_close(v, SCR.sample_smooth_channels(image, p, rot, trans), 1e-10, "values")
        _check_pullback(pb, SCR.sample_smooth_channels_pullback(dv, image, p, rot, trans), np.float64)
        res.append((v,) + tuple(pb))
    scale = max(float(a.abs().max()) for a in res[0][1:])
    for name, a, b in zip(("values",) + FIELDS, *res):
        assert float((a - b).abs().max()) < 1e-6 * scale, name


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_no_poses_one_point_and_a_nan_point(dev, algo, npdt, tdt, n_in, n_out):
    rng = np.random.default_rng(13)
    B, C, grid = 3, 5, (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    image = rng.normal(size=grid + (C, B))
    img, R, t = grid_to_dev(image.astype(npdt), dev), T(rot.astype(npdt), dev), T(trans.astype(npdt), dev)
    pull = dpr_amd.sample_smooth_channels_pullback_
    z = lambda *sh: torch.zeros(sh, dtype=tdt, device=dev)
    # P = 0: empty values; every gradient is zero
    none = z(0, n_in)
    assert dpr_amd.sample_smooth_channels(img, none, R, t).shape == (0, C, B)
    pb = pull(z(B, 0, C).permute(1, 2, 0), img, none, R, t, algo=algo)
    assert pb.points.shape == (0, n_in) and pb.image.shape == grid + (C, B)
    for g in (pb.image, pb.rotation, pb.translation):
        assert bool((g == 0).all())
    # B = 0: empty values, images and pose gradients, zero point gradients
    pts5 = T(rng.uniform(-1.0, 1.0, size=(5, n_in)).astype(npdt), dev)
    img0 = dpr_amd.empty_channel_grid(grid, C, 0, tdt, dev)
    assert dpr_amd.sample_smooth_channels(img0, pts5, z(0, n_out, n_in), z(0, n_out)).shape == (5, C, 0)
    nan = torch.full((5, n_in), float("nan"), dtype=tdt, device=dev)
    pb = pull(z(0, 5, C).permute(1, 2, 0), img0, pts5, z(0, n_out, n_in), z(0, n_out), ds_dpoints=nan, algo=algo)
    assert pb.rotation.shape == (0, n_out, n_in) and pb.image.shape == grid + (C, 0) and pb.points is nan
    assert bool((nan == 0).all())
    # one point
    one = np.full((1, n_in), 0.21)
    dv1 = rng.normal(size=(1, C, B))
    v = dpr_amd.sample_smooth_channels(img, T(one.astype(npdt), dev), R, t)
    assert_close(v, SCR.sample_smooth_channels(image, one, rot, trans).astype(npdt), tol(npdt, "points"), "one point")
    pb = pull(_values_to_dev(dv1.astype(npdt), dev), img, T(one.astype(npdt), dev), R, t, algo=algo)
    _check_pullback(pb, SCR.sample_smooth_channels_pullback(dv1, image, one, rot, trans), npdt, "one point ")
    # a NaN point: value 0, no deposit, and no gradient hears of it; the other points as without it
    pts = rng.uniform(-1.0, 1.0, size=(5, n_in))
    pts[2, 0] = np.nan
    dv = rng.normal(size=(5, C, B))
    keep = [0, 1, 3, 4]
    v = dpr_amd.sample_smooth_channels(img, T(pts.astype(npdt), dev), R, t)
    assert bool((v[2] == 0).all()) and bool(torch.isfinite(v).all())
    assert torch.equal(v[keep], dpr_amd.sample_smooth_channels(img, T(pts[keep].astype(npdt), dev), R, t))
    pb = pull(_values_to_dev(dv.astype(npdt), dev), img, T(pts.astype(npdt), dev), R, t, algo=algo)
    ref = SCR.sample_smooth_channels_pullback(dv[keep], image, pts[keep], rot, trans)
    assert bool((pb.points[2] == 0).all())
    _check_pullback((pb.image, pb.points[keep], pb.rotation, pb.translation), ref, npdt, "NaN point ")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_need_subsets_write_only_their_buffers(dev, algo, npdt, tdt):
    """The four outputs lie back to back in one arena filled with 7.5: a call writes the ones in `need`, returns
    them by identity, and leaves every other byte of the arena alone."""
    n_in, n_out, B, C, P, grid = 3, 3, 3, 3, 300, (8, 8, 8)
    rng = np.random.default_rng(17)
    rot, trans = _poses(rng, B, n_in, n_out)
    image, pts = rng.normal(size=grid + (C, B)), rng.uniform(-1.15, 1.15, size=(P, n_in))
    dv = rng.normal(size=(P, C, B))
    img, p, R, t = grid_to_dev(image.astype(npdt), dev), T(pts.astype(npdt), dev), T(rot.astype(npdt), dev), \
        T(trans.astype(npdt), dev)
    dvd = _values_to_dev(dv.astype(npdt), dev)
    ref = SCR.sample_smooth_channels_pullback(dv, image, pts, rot, trans)
    G = int(np.prod(grid))
    sizes = dict(image=B * C * G, points=P * n_in, rotation=B * n_in * n_out, translation=B * n_out)
    for need in (("image",), ("points",), ("rotation",), ("translation",), ("rotation", "translation"),
                 ("image", "points"), FIELDS):
        arena = torch.full((sum(sizes.values()),), 7.5, dtype=tdt, device=dev)
        parts, o = {}, 0
        for name in FIELDS:
            parts[name] = arena[o:o + sizes[name]]
            o += sizes[name]
        bufs = dict(image=parts["image"].view((B, C) + grid[::-1]).permute(4, 3, 2, 1, 0),
                    points=parts["points"].view(P, n_in),
                    rotation=parts["rotation"].view(B, n_in, n_out).transpose(1, 2),
                    translation=parts["translation"].view(B, n_out))
        pb = dpr_amd.sample_smooth_channels_pullback_(dvd, img, p, R, t, need=need, algo=algo,
                                                      **{f"ds_d{name}": bufs[name] for name in need})
        for name, kind, e in zip(FIELDS, KINDS, ref):
            got = getattr(pb, name)
            if name in need:
                assert got.data_ptr() == bufs[name].data_ptr()
                assert_close(got, e.astype(npdt), tol(npdt, kind), f"{need}: {name}")
            else:
                assert got is None
                assert bool((parts[name] == 7.5).all()), f"{need}: {name} was written"


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
def test_image_gradient_without_the_image(dev, algo):
    c = _case(3, 2)
    npdt, C = np.float32, 5
    _img, pts, rot, trans = _dev_args(c, dev, npdt, C, NB)
    dv = _values_to_dev(c["dv"][:, :C].astype(npdt), dev)
    want = _ref_pullback(c, C, NB)[0].astype(npdt)
    pull = dpr_amd.sample_smooth_channels_pullback_
    pb = pull(dv, None, pts, rot, trans, need=("image",), algo=algo, grid_size=c["grid"])
    assert_close(pb.image, want, tol(npdt, "out"), "image=None, grid_size")
    pb = pull(dv, None, pts, rot, trans, need=("image",), algo=algo, grid_size=c["grid"], channels=C)
    assert_close(pb.image, want, tol(npdt, "out"), "image=None, grid_size, channels")
    buf = dpr_amd.empty_channel_grid(c["grid"], C, NB, torch.float32, dev)
    pb = pull(dv, None, pts, rot, trans, need=("image",), algo=algo, ds_dimage=buf)
    assert pb.image is buf
    assert_close(buf, want, tol(npdt, "out"), "image=None, ds_dimage")
    with pytest.raises(ValueError):
        pull(dv, None, pts, rot, trans, algo=algo, grid_size=c["grid"])
    with pytest.raises(ValueError):
        pull(dv, None, pts, rot, trans, need=("image",), algo=algo)
    # contradictory shapes
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv, None, pts, rot, trans, need=("image",), algo=algo, grid_size=c["grid"], channels=C + 1)
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv, None, pts, rot, trans, need=("image",), algo=algo,
             ds_dimage=dpr_amd.empty_channel_grid(c["grid"], C - 1, NB, torch.float32, dev))
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv[:, :C - 1], _img, pts, rot, trans, algo=algo)
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv, _img, pts, rot, trans, algo=algo, channels=C - 1)


def test_refused_calls_leave_their_outputs_untouched(dev):
    c = _case(3, 3)
    P, B, C, grid = len(c["points"]), 2, 4, c["grid"]
    img, pts, rot, trans = _dev_args(c, dev, np.float32, C, B)
    dv = _values_to_dev(c["dv"][:, :C, :B].astype(np.float32), dev)
    sentinel = torch.full((B, P, C), 7.5, device=dev).permute(1, 2, 0)
    for algo in ("tiled", "chunked", "ordered"):
        with pytest.raises(dpr_amd.DprError) as e:
            dpr_amd.sample_smooth_channels_(sentinel, img, pts, rot, trans, algo=algo)
        assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.sample_smooth_channels_(sentinel, img[..., :1], pts, rot, trans)
    with pytest.raises(dpr_amd.DimensionMismatch):  # C of the image and of `values` differ
        dpr_amd.sample_smooth_channels_(sentinel, dpr_amd.to_grid_layout(img[..., :3, :]), pts, rot, trans)
    with pytest.raises(ValueError):  # the wrong memory order: (P, C, B) contiguous
        dpr_amd.sample_smooth_channels_(torch.full((P, C, B), 7.5, device=dev), img, pts, rot, trans)
    with pytest.raises(dpr_amd.DprError) as e:  # C = 17 from the image
        dpr_amd.sample_smooth_channels(dpr_amd.empty_channel_grid(grid, 17, B, torch.float32, dev), pts, rot, trans)
    assert e.value.code == _lib.ERR_INVALID_ARG
    d_img = dpr_amd.empty_channel_grid(grid, C, B, torch.float32, dev).fill_(7.5)
    d_pts = torch.full((P, 3), 7.5, device=dev)
    for algo in ("chunked", "ordered"):
        with pytest.raises(dpr_amd.DprError) as e:
            dpr_amd.sample_smooth_channels_pullback_(dv, img, pts, rot, trans, need=("image", "points"),
                                                     ds_dimage=d_img, ds_dpoints=d_pts, algo=algo)
        assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    # C level, real device buffers: C = 0 and 17, a TILED forward, KEEP / REUSE, a workspace 256 bytes too small for
    # the tiled pullback, one misaligned, a misaligned output
    g = np.asarray(grid, dtype=np.int64)
    gp = g.ctypes.data_as(ctypes.c_void_p)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    L = _lib.lib()
    need = int(L.dpr_workspace_bytes_sample_smooth_channels_ex_f32(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, 3, 3, gp, P, B,
                                                                   C))
    assert need > 256 and need % 256 == 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    dvc, vc, rot_cm = dv.permute(2, 0, 1), sentinel.permute(2, 0, 1), rot.transpose(1, 2).contiguous()
    assert dvc.is_contiguous() and vc.is_contiguous()

    def fwd(algo, flags, C_):
        return L.dpr_sample_smooth_channels_ex_f32(None, algo, flags, 3, 3, gp, P, B, C_, ptr(vc), ptr(img), ptr(pts),
                                                   ptr(rot_cm), ptr(trans), None, 0)

    def bwd(algo, flags, C_, d_img_ptr, ws_ptr, ws_bytes):
        return L.dpr_sample_smooth_channels_pullback_ex_f32(None, algo, flags, 3, 3, gp, P, B, C_, ptr(dvc), ptr(img),
                                                            ptr(pts), ptr(rot_cm), ptr(trans), d_img_ptr, ptr(d_pts),
                                                            None, None, ws_ptr, ws_bytes)

    for C_ in (0, 17):
        assert fwd(_lib.ALGO_ATOMIC, 0, C_) == _lib.ERR_INVALID_ARG
        assert bwd(_lib.ALGO_ATOMIC, 0, C_, ptr(d_img), None, 0) == _lib.ERR_INVALID_ARG
        assert "channels C" in _lib.last_error()
    assert fwd(_lib.ALGO_TILED, 0, C) == _lib.ERR_UNSUPPORTED_ALGO
    for flags in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
        assert fwd(_lib.ALGO_ATOMIC, flags, C) == _lib.ERR_UNSUPPORTED_ALGO
        assert bwd(_lib.ALGO_ATOMIC, flags, C, ptr(d_img), None, 0) == _lib.ERR_UNSUPPORTED_ALGO
    assert bwd(_lib.ALGO_TILED, 0, C, ptr(d_img), None, 0) == _lib.ERR_WORKSPACE
    assert bwd(_lib.ALGO_TILED, 0, C, ptr(d_img), ptr(ws), need - 256) == _lib.ERR_WORKSPACE
    assert "workspace" in _lib.last_error()
    assert bwd(_lib.ALGO_TILED, 0, C, ptr(d_img), ctypes.c_void_p(ws.data_ptr() + 64), need) == _lib.ERR_WORKSPACE
    assert "256-byte aligned" in _lib.last_error()
    assert bwd(_lib.ALGO_ATOMIC, 0, C, ctypes.c_void_p(d_img.data_ptr() + 2), None, 0) == _lib.ERR_INVALID_ARG
    with pytest.raises(ValueError):  # the Python wrapper checks the workspace it is given
        dpr_amd.sample_smooth_channels_pullback_(dv, img, pts, rot, trans, need=("image", "points"), ds_dimage=d_img,
                                                 ds_dpoints=d_pts, algo="tiled", workspace=ws[:need - 256])
    torch.cuda.synchronize()
    assert bool((sentinel == 7.5).all()) and bool((d_img == 7.5).all()) and bool((d_pts == 7.5).all())


# ------------------------------------------------------------------ the workspace and stream contract
GUARD, GUARD_BYTE = 4096, 0xA5


@pytest.mark.parametrize("npdt,tdt,suf", [(np.float32, torch.float32, "f32"), (np.float64, torch.float64, "f64")])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_workspace_contents_do_not_matter_and_nothing_is_written_outside(dev, npdt, tdt, suf, n_in, n_out):
    """The TILED pullback on the interior of a buffer with two guard bands of 4096 bytes, from a zeroed workspace and
    from one with every byte 0xFF (the all-ones key, the largest index and count): the guards stay, the outputs
    (pre-filled with NaN) match the reference either way."""
    c = _case(n_in, n_out)
    C, P, grid = 5, len(c["points"]), c["grid"]
    args = _dev_args(c, dev, npdt, C, NB)
    dv = _values_to_dev(c["dv"][:, :C].astype(npdt), dev)
    g = np.asarray(grid, dtype=np.int64)
    need = int(getattr(_lib.lib(), f"dpr_workspace_bytes_sample_smooth_channels_ex_{suf}")(
        _lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, g.ctypes.data_as(ctypes.c_void_p), P, NB, C))
    assert need > 0 and need % 256 == 0
    buf = torch.full((need + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    band = torch.full((GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    e = lambda *sh: torch.empty(sh, dtype=tdt, device=dev)
    outs = dict(ds_dimage=dpr_amd.empty_channel_grid(grid, C, NB, tdt, dev), ds_dpoints=e(P, n_in),
                ds_drotation=e(NB, n_in, n_out).transpose(1, 2), ds_dtranslation=e(NB, n_out))
    ref = _ref_pullback(c, C, NB)
    for pattern in ("zeros", "ones"):
        ws.fill_(0 if pattern == "zeros" else 0xFF)
        for t in outs.values():
            t.fill_(float("nan"))
        pb = dpr_amd.sample_smooth_channels_pullback_(dv, *args, algo="tiled", workspace=ws, **outs)
        torch.cuda.synchronize()
        assert torch.equal(buf[:GUARD], band), f"{pattern}: bytes in front of the workspace were overwritten"
        assert torch.equal(buf[GUARD + need:], band), f"{pattern}: bytes behind the {need} queried were overwritten"
        for name, t in outs.items():
            assert bool(torch.isfinite(t).all()), f"{pattern}: {name} holds NaN / Inf (or was not overwritten)"
        _check_pullback(pb, ref, npdt, f"{pattern}: ")


class Calls:
    """Forward and pullback on device buffers that stay where they are (fp32, 8^N grid, 300 points, B = 3, C = 5)."""
    P, B, C = 300, 3, 5

    def __init__(self, dev, n_in, n_out, algos):
        self.dev, self.n_in, self.n_out, self.algos = dev, n_in, n_out, algos
        self.grid = (8,) * n_out
        P, B, C = self.P, self.B, self.C
        e = lambda *sh: torch.empty(sh, device=dev)
        self.inp = [dpr_amd.empty_channel_grid(self.grid, C, B, torch.float32, dev), e(P, n_in), e(B, n_out, n_in),
                    e(B, n_out), e(B, P, C).permute(1, 2, 0)]  # image, points, rotation, translation, ds_dvalues
        self.values = e(B, P, C).permute(1, 2, 0)
        self.grads = {a: dict(ds_dimage=dpr_amd.empty_channel_grid(self.grid, C, B, torch.float32, dev),
                              ds_dpoints=e(P, n_in), ds_drotation=e(B, n_in, n_out).transpose(1, 2),
                              ds_dtranslation=e(B, n_out)) for a in algos}
        self.staged, self.refs = {}, {}

    def problem(self, seed):
        rng = np.random.default_rng(seed)
        rot, trans = _poses(rng, self.B, self.n_in, self.n_out)
        return [rng.normal(size=self.grid + (self.C, self.B)), rng.uniform(-1.15, 1.15, size=(self.P, self.n_in)),
                rot, trans, rng.normal(size=(self.P, self.C, self.B))]

    def stage(self, *seeds):
        for seed in seeds:
            image, pts, rot, trans, dv = self.problem(seed)
            f = np.float32
            self.staged[seed] = [grid_to_dev(image.astype(f), self.dev), T(pts.astype(f), self.dev),
                                 T(rot.astype(f), self.dev), T(trans.astype(f), self.dev),
                                 _values_to_dev(dv.astype(f), self.dev)]
            self.refs[seed] = (SCR.sample_smooth_channels(image, pts, rot, trans),
                               SCR.sample_smooth_channels_pullback(dv, image, pts, rot, trans))
        torch.cuda.synchronize()

    def poison(self, inputs=False):
        for v in [self.values] + [t for g in self.grads.values() for t in g.values()] + (self.inp if inputs else []):
            v.fill_(float("nan"))

    def load(self, seed):
        for dst, src in zip(self.inp, self.staged[seed]):
            dst.copy_(src, non_blocking=True)

    def run(self):
        dpr_amd.sample_smooth_channels_(self.values, *self.inp[:4])
        self.pb = {a: dpr_amd.sample_smooth_channels_pullback_(self.inp[4], *self.inp[:4], algo=a, **self.grads[a])
                   for a in self.algos}

    def check(self, seed, what):
        values, ref = self.refs[seed]
        assert_close(self.values, values.astype(np.float32), tol(np.float32, "points"), f"{what}: values")
        for a, pb in self.pb.items():
            _check_pullback(pb, ref, np.float32, f"{what}: {a} ")


@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2)])
def test_runs_on_the_callers_stream(dev, n_in, n_out):
    """The inputs start as NaN; on a side stream a filler, the copies of the real inputs, the calls (both pullback
    algorithms).  A launch or zeroing on another stream would not wait for them.  (Can pass by luck of timing, never
    fail by it.)"""
    c = Calls(dev, n_in, n_out, ("atomic", "tiled"))
    c.poison(inputs=True)
    c.stage(4)
    a = torch.randn(4096, 4096, device=dev)
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(4):  # (a few milliseconds on the side stream)
            torch.matmul(a, a, out=b)
        c.load(4)
        c.run()
    side.synchronize()
    c.check(4, "side stream")


def test_atomic_calls_are_captured_into_a_hip_graph_and_replayed_on_new_contents(dev):
    c = Calls(dev, 3, 3, ("atomic",))
    c.stage(4, 5)
    c.load(4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c.run()  # warm-up outside the capture
    side.synchronize()
    c.check(4, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one capture, one stream, no fork
        c.run()
    for seed, what in ((5, "graph replay on new contents"), (4, "second replay, on the first contents")):
        c.load(seed)
        c.poison()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        c.check(seed, what)
