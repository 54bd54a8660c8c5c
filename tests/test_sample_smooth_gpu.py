"""Smooth sampling on the GPU (dpr_amd.sample_smooth / sample_smooth_pullback_ / sample_smooth_ad) against the numpy
reference tests/sample_smooth_reference.py evaluated in fp64.  The interpolant is C1, so a different fp32 cell choice
changes nothing at first order and no same-precision oracle is needed.  Tolerances: the project's norm-wise ones
(tests/test_parity_gpu.py: fp64 1e-10; fp32 5e-5 "out" for ds_dimage, 1e-4 "points" for values -- the sum
tests/test_smooth_gpu.py holds as ds_dpoint_weight to that bound -- and ds_dpoints, 1e-3 "pose" for ds_drotation and
ds_dtranslation).

The hard-regime cloud and grids are those of tests/test_smooth_gpu.py ((150, 37) and (37, 19, 21): three tiles and a
partial last tile per axis of the tiled path, rejected points, halo and dropped cells, 2 000 points in one cell,
corner-cell centres)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests import sample_smooth_reference as SSR
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol
from tests.test_smooth_gpu import _case as _smooth_case
from tests.test_smooth_gpu import _poses

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
FIELDS = ("image", "points", "rotation", "translation")
KINDS = ("out", "points", "pose", "pose")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out):
    """The cloud and poses of tests/test_smooth_gpu.py with an image and value gradients, and the fp64 reference
    results for B = 3 and B = 1, computed once and shared; never modified."""
    s = _smooth_case(n_in, n_out)
    rng = np.random.default_rng(1000 + 10 * n_in + n_out)
    P = len(s["points"])
    c = dict(grid=s["grid"], points=s["points"], rot=s["rot"], trans=s["trans"],
             image=rng.normal(size=s["grid"] + (3,)), dv=rng.normal(size=(P, 3)))
    for B in (3, 1):
        a = (c["image"][..., :B], c["points"], c["rot"][:B], c["trans"][:B])
        c["values", B] = SSR.sample_smooth(*a)
        c["pb", B] = SSR.sample_smooth_pullback(c["dv"][:, :B], *a)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _values_to_dev(a, dev):
    """numpy (P, B) -> device tensor with the point index fastest."""
    return T(np.ascontiguousarray(a.T), dev).t()


def _dev_args(c, dev, npdt, B):
    return [grid_to_dev(c["image"][..., :B].astype(npdt), dev), T(c["points"].astype(npdt), dev),
            T(c["rot"][:B].astype(npdt), dev), T(c["trans"][:B].astype(npdt), dev)]


def _check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ the hard-regime cloud
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_matches_the_reference(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    P = len(c["points"])
    # pose 0 (the identity) does reach the branches the cloud is built for: points at least 1e-3 of a cell outside
    # the accepted range, and accepted points within 1.5 cells of the border (a dropped cell)
    n = np.asarray(c["grid"], dtype=np.float64)
    coord = (c["points"][:, :n_out] + 1) * n / 2
    rejected = np.any((coord < -1 - 1e-3) | (coord > n + 1 + 1e-3), axis=1)
    accepted = np.all((coord >= -1) & (coord < n + 1), axis=1)
    dropping = accepted & np.any((coord < 1) | (coord >= n - 1), axis=1)
    assert rejected.sum() > 100 and dropping.sum() > 100
    assert np.all(c["values", 3][rejected, 0] == 0) and np.all(c["values", 3][dropping, 0] != 0)
    for B in (3, 1):
        v = dpr_amd.sample_smooth(*_dev_args(c, dev, npdt, B))
        assert v.shape == (P, B) and v.dtype == tdt and v.t().is_contiguous()
        assert_close(v, c["values", B].astype(npdt), tol(npdt, "points"), f"B={B}")
        assert bool((v[torch.as_tensor(rejected, device=dev), 0] == 0).all())
    # single pose: a vector
    img, pts, rot, trans = _dev_args(c, dev, npdt, 1)
    v = dpr_amd.sample_smooth(dpr_amd.to_grid_layout(img[..., 0]), pts, rot[0], trans[0], algo="atomic")
    assert v.shape == (P,)
    assert_close(v, c["values", 1][:, 0].astype(npdt), tol(npdt, "points"), "single pose")


@pytest.mark.parametrize("algo", ["atomic", "tiled", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    for B in (3, 1):
        dv = _values_to_dev(c["dv"][:, :B].astype(npdt), dev)
        pb = dpr_amd.sample_smooth_pullback_(dv, *_dev_args(c, dev, npdt, B), algo=algo)
        assert pb.image.shape == c["grid"] + (B,) and pb.points.dtype == tdt
        assert pb.rotation.shape == (B, n_out, n_in) and pb.translation.shape == (B, n_out)
        _check_pullback(pb, c["pb", B], npdt, f"{algo} B={B} ")
    # single pose: unbatched results
    img, pts, rot, trans = _dev_args(c, dev, npdt, 1)
    p1 = dpr_amd.sample_smooth_pullback_(T(c["dv"][:, 0].astype(npdt), dev), dpr_amd.to_grid_layout(img[..., 0]), pts,
                                         rot[0], trans[0], algo=algo)
    assert p1.image.shape == c["grid"] and p1.rotation.shape == (n_out, n_in) and p1.translation.shape == (n_out,)
    ref = c["pb", 1]
    _check_pullback(p1, (ref[0][..., 0], ref[1], ref[2][0], ref[3][0]), npdt, f"{algo} single pose ")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_image_planes_are_the_tiled_smooth_forward(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    img, pts, rot, trans = _dev_args(c, dev, npdt, 3)
    dv = _values_to_dev(c["dv"].astype(npdt), dev)
    pb = dpr_amd.sample_smooth_pullback_(dv, img, pts, rot, trans, need=("image",), algo="tiled")
    assert pb.points is None and pb.rotation is None and pb.translation is None
    for b in range(3):
        want = dpr_amd.raster_smooth(c["grid"], pts, rot[b], trans[b], point_weight=dv[:, b].contiguous(),
                                     algo="tiled")
        assert_close(pb.image[..., b], want.cpu().numpy(), tol(npdt, "out"), f"plane {b}")


# ------------------------------------------------------------------ pose slicing
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_many_poses_of_a_small_cloud(dev, npdt, tdt, n_in, n_out):
    """B = 70, P = 300 on an 8^N grid: two blocks of points, so the launch cuts the poses into 70 slices of one pose
    each (tests/test_sample_smooth_hard_gpu.py has several poses per slice)."""
    rng = np.random.default_rng(7)
    B, P, grid = 70, 300, (8,) * n_out
    pts = rng.uniform(-1.15, 1.15, size=(P, n_in))
    rot, trans = _poses(rng, B, n_in, n_out)
    image, dv = rng.normal(size=grid + (B,)), rng.normal(size=(P, B))
    a = [grid_to_dev(image.astype(npdt), dev)] + [T(x.astype(npdt), dev) for x in (pts, rot, trans)]
    v = dpr_amd.sample_smooth(*a)
    assert_close(v, SSR.sample_smooth(image, pts, rot, trans).astype(npdt), tol(npdt, "points"), "B=70 values")
    ref = SSR.sample_smooth_pullback(dv, image, pts, rot, trans)
    for algo in ("atomic", "tiled"):
        pb = dpr_amd.sample_smooth_pullback_(_values_to_dev(dv.astype(npdt), dev), *a, algo=algo)
        _check_pullback(pb, ref, npdt, f"B=70 {algo} ")


# ------------------------------------------------------------------ derivative tests on the device
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, n_in, n_out):
    """sample_smooth_ad in fp64 on an 8^N grid with 10 points and B = 2: central differences with h = 1e-6 of
    sum(values * dv) in image, points, rotation and translation, within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_reference.py)."""
    rng = np.random.default_rng(11)
    B, P, grid = 2, 10, (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    vals = [rng.normal(size=grid + (B,)), rng.uniform(-1.1, 1.1, size=(P, n_in)), rot, trans]
    dv = T(rng.normal(size=(P, B)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    (dpr_amd.sample_smooth_ad(*xs) * dv).sum().backward()
    grads = [x.grad.cpu().numpy() for x in xs]
    scale = max(np.abs(a).max() for a in grads)
    h = 1e-6
    with torch.no_grad():
        for k, (x, ga) in enumerate(zip(xs, grads)):
            flat = x.view(-1)
            fd = np.zeros(flat.numel())
            for i in range(flat.numel()):
                keep = float(flat[i])
                flat[i] = keep + h
                up = float((dpr_amd.sample_smooth(*xs) * dv).sum())
                flat[i] = keep - h
                dn = float((dpr_amd.sample_smooth(*xs) * dv).sum())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (FIELDS[k], err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_values_and_gradients_are_continuous_across_a_cell_boundary(dev, n_in, n_out):
    """Points 1e-9 of a cell either side of an integer coord (fp64): values and all four gradients differ by less
    than 1e-6 * max|gradient|, and agree with the reference on both sides."""
    rng = np.random.default_rng(5)
    grid = (8,) * n_out
    image = rng.normal(size=grid + (1,))
    rot, trans = np.eye(n_out, n_in)[None], np.zeros((1, n_out))
    base = rng.uniform(-0.5, 0.5, size=(6, n_in))
    base[:, 0] = -1 + 2.0 * np.array([2, 3, 4, 5, 6, 3]) / grid[0]
    lo, hi = base.copy(), base.copy()
    lo[:, 0] -= 1e-9 * 2 / grid[0]
    hi[:, 0] += 1e-9 * 2 / grid[0]
    assert np.all(np.floor((lo[:, 0] + 1) * 4) + 1 == np.floor((hi[:, 0] + 1) * 4))
    dv = rng.normal(size=(6, 1))
    img_d, dv_d = grid_to_dev(image, dev), _values_to_dev(dv, dev)
    res = []
    for p in (lo, hi):
        a = (T(p, dev), T(rot, dev), T(trans, dev))
        v = dpr_amd.sample_smooth(img_d, *a)
        pb = dpr_amd.sample_smooth_pullback_(dv_d, img_d, *a)
        assert_close(v, SSR.sample_smooth(image, p, rot, trans), 1e-10, "values")
        _check_pullback(pb, SSR.sample_smooth_pullback(dv, image, p, rot, trans), np.float64)
        res.append((v,) + tuple(pb))
    scale = max(float(a.abs().max()) for a in res[0][1:])
    for name, a, b in zip(("values",) + FIELDS, *res):
        assert float((a - b).abs().max()) < 1e-6 * scale, name


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_one_point_and_a_nan_point(dev, algo, npdt, tdt, n_in, n_out):
    rng = np.random.default_rng(13)
    B, grid = 3, (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    image = rng.normal(size=grid + (B,))
    img, R, t = grid_to_dev(image.astype(npdt), dev), T(rot.astype(npdt), dev), T(trans.astype(npdt), dev)
    # P = 0: empty values; every gradient is zero
    none = torch.zeros((0, n_in), dtype=tdt, device=dev)
    assert dpr_amd.sample_smooth(img, none, R, t).shape == (0, B)
    pb = dpr_amd.sample_smooth_pullback_(torch.zeros((B, 0), dtype=tdt, device=dev).t(), img, none, R, t, algo=algo)
    assert pb.points.shape == (0, n_in)
    for g in (pb.image, pb.rotation, pb.translation):
        assert bool((g == 0).all())
    # one point
    one = np.full((1, n_in), 0.21)
    dv1 = rng.normal(size=(1, B))
    v = dpr_amd.sample_smooth(img, T(one.astype(npdt), dev), R, t)
    assert_close(v, SSR.sample_smooth(image, one, rot, trans).astype(npdt), tol(npdt, "points"), "one point")
    pb = dpr_amd.sample_smooth_pullback_(_values_to_dev(dv1.astype(npdt), dev), img, T(one.astype(npdt), dev), R, t,
                                         algo=algo)
    _check_pullback(pb, SSR.sample_smooth_pullback(dv1, image, one, rot, trans), npdt, "one point ")
    # a NaN point: value 0, and no gradient hears of it
    pts = rng.uniform(-1.0, 1.0, size=(5, n_in))
    pts[2, 0] = np.nan
    dv = rng.normal(size=(5, B))
    keep = [0, 1, 3, 4]
    v = dpr_amd.sample_smooth(img, T(pts.astype(npdt), dev), R, t)
    assert bool((v[2] == 0).all()) and bool(torch.isfinite(v).all())
    pb = dpr_amd.sample_smooth_pullback_(_values_to_dev(dv.astype(npdt), dev), img, T(pts.astype(npdt), dev), R, t,
                                         algo=algo)
    ref = SSR.sample_smooth_pullback(dv[keep], image, pts[keep], rot, trans)
    assert bool((pb.points[2] == 0).all())
    assert_close(pb.points[keep], ref[1].astype(npdt), tol(npdt, "points"), "NaN point: points")
    _check_pullback((pb.image, pb.points[keep], pb.rotation, pb.translation), ref, npdt, "NaN point ")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_need_subsets_write_only_their_buffers(dev, algo, npdt, tdt):
    """The four outputs lie back to back in one arena filled with 7.5: a call writes the ones in `need`, returns
    them by identity, and leaves every other byte of the arena alone."""
    n_in, n_out, B, P, grid = 3, 3, 3, 300, (8, 8, 8)
    rng = np.random.default_rng(17)
    rot, trans = _poses(rng, B, n_in, n_out)
    image, pts, dv = rng.normal(size=grid + (B,)), rng.uniform(-1.15, 1.15, size=(P, n_in)), rng.normal(size=(P, B))
    img, p, R, t = grid_to_dev(image.astype(npdt), dev), T(pts.astype(npdt), dev), T(rot.astype(npdt), dev), \
        T(trans.astype(npdt), dev)
    dvd = _values_to_dev(dv.astype(npdt), dev)
    ref = SSR.sample_smooth_pullback(dv, image, pts, rot, trans)
    G = int(np.prod(grid))
    sizes = dict(image=B * G, points=P * n_in, rotation=B * n_in * n_out, translation=B * n_out)
    for need in (("image",), ("points",), ("rotation",), ("translation",), ("rotation", "translation"),
                 ("image", "points"), FIELDS):
        arena = torch.full((sum(sizes.values()),), 7.5, dtype=tdt, device=dev)
        parts, o = {}, 0
        for name in FIELDS:
            parts[name] = arena[o:o + sizes[name]]
            o += sizes[name]
        bufs = dict(image=parts["image"].view((B,) + grid[::-1]).permute(3, 2, 1, 0),
                    points=parts["points"].view(P, n_in),
                    rotation=parts["rotation"].view(B, n_in, n_out).transpose(1, 2),
                    translation=parts["translation"].view(B, n_out))
        pb = dpr_amd.sample_smooth_pullback_(dvd, img, p, R, t, need=need, algo=algo,
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
    npdt = np.float32
    _img, pts, rot, trans = _dev_args(c, dev, npdt, 3)
    dv = _values_to_dev(c["dv"].astype(npdt), dev)
    pb = dpr_amd.sample_smooth_pullback_(dv, None, pts, rot, trans, need=("image",), algo=algo, grid_size=c["grid"])
    assert_close(pb.image, c["pb", 3][0].astype(npdt), tol(npdt, "out"), "image=None, grid_size")
    buf = dpr_amd.empty_grid(c["grid"], 3, torch.float32, dev)
    pb = dpr_amd.sample_smooth_pullback_(dv, None, pts, rot, trans, need=("image",), algo=algo, ds_dimage=buf)
    assert pb.image is buf
    assert_close(buf, c["pb", 3][0].astype(npdt), tol(npdt, "out"), "image=None, ds_dimage")
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_pullback_(dv, None, pts, rot, trans, algo=algo, grid_size=c["grid"])
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_pullback_(dv, None, pts, rot, trans, need=("image",), algo=algo)


def test_refused_calls_leave_their_outputs_untouched(dev):
    c = _case(3, 3)
    P, B, grid = len(c["points"]), 2, c["grid"]
    img, pts, rot, trans = _dev_args(c, dev, np.float32, B)
    dv = _values_to_dev(c["dv"][:, :B].astype(np.float32), dev)
    sentinel = torch.full((B, P), 7.5, device=dev).t()
    for algo in ("tiled", "chunked", "ordered"):
        with pytest.raises(dpr_amd.DprError) as e:
            dpr_amd.sample_smooth_(sentinel, img, pts, rot, trans, algo=algo)
        assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.sample_smooth_(sentinel, img[..., :1], pts, rot, trans)
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_(torch.full((P, B), 7.5, device=dev), img, pts, rot, trans)
    d_img = dpr_amd.empty_grid(grid, B, torch.float32, dev).fill_(7.5)
    d_pts = torch.full((P, 3), 7.5, device=dev)
    for algo in ("chunked", "ordered"):
        with pytest.raises(dpr_amd.DprError) as e:
            dpr_amd.sample_smooth_pullback_(dv, img, pts, rot, trans, need=("image", "points"), ds_dimage=d_img,
                                            ds_dpoints=d_pts, algo=algo)
        assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    # C level, real device buffers: KEEP / REUSE, a workspace too small for the tiled pullback, one misaligned, a
    # misaligned output
    g = np.asarray(grid, dtype=np.int64)
    gp = g.ctypes.data_as(ctypes.c_void_p)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    fn = _lib.lib().dpr_sample_smooth_pullback_ex_f32
    need = dpr_amd.workspace_bytes_sample_smooth("pullback", grid, P, B, 3, algo="tiled")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    dvc, rot_cm = dv.t().contiguous(), rot.transpose(1, 2).contiguous()

    def call(algo, flags, d_img_ptr, ws_ptr, ws_bytes):
        return fn(None, algo, flags, 3, 3, gp, P, B, ptr(dvc), ptr(img), ptr(pts), ptr(rot_cm), ptr(trans), d_img_ptr,
                  ptr(d_pts), None, None, ws_ptr, ws_bytes)

    for flags in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
        assert call(_lib.ALGO_ATOMIC, flags, ptr(d_img), None, 0) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(_lib.ALGO_TILED, 0, ptr(d_img), None, 0) == _lib.ERR_WORKSPACE
    assert call(_lib.ALGO_TILED, 0, ptr(d_img), ptr(ws), need - 1) == _lib.ERR_WORKSPACE
    assert "workspace" in _lib.last_error()
    assert call(_lib.ALGO_TILED, 0, ptr(d_img), ctypes.c_void_p(ws.data_ptr() + 64), need) == _lib.ERR_WORKSPACE
    assert "256-byte aligned" in _lib.last_error()
    assert call(_lib.ALGO_ATOMIC, 0, ctypes.c_void_p(d_img.data_ptr() + 2), None, 0) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((sentinel == 7.5).all()) and bool((d_img == 7.5).all()) and bool((d_pts == 7.5).all())
