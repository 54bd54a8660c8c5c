"""The smooth splat on the GPU (dpr_amd.raster_smooth / raster_pullback_smooth_ / raster_smooth_ad) against the numpy
reference tests/smooth_reference.py evaluated in fp64.  The operator is C1, so a different fp32 cell choice changes
nothing at first order and no same-precision oracle is needed.  Tolerances: the project's norm-wise ones
(tests/test_parity_gpu.py: fp64 1e-10; fp32 5e-5 `out`, 1e-4 point gradients, 1e-3 pose gradients).

Shapes: the grids have three tiles and a partial last tile on every axis of the tiled forward's tiles (3-D 16 x 8 x 8:
(37, 19, 21); 2-D 64 x 16: (150, 37)).  The cloud: 20 000 points uniform in +-1.15 (rejected points, halo cells
outside the grid and dropped cells all occur) with the slab 0.7 <= x_0 left empty (pose 0 is the identity: its last
tile layer along axis 0 holds no point of the uniform part), 2 000 points packed into one cell, and one point at the
centre of each corner cell of the grid."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests import smooth_reference as SR
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (150, 37), 3: (37, 19, 21)}
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _poses(rng, B, n_in, n_out):
    """Pose 0: the identity; the others: random rotations (rows of an orthogonal matrix) and small shifts."""
    q, _ = np.linalg.qr(rng.normal(size=(B, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :n_out, :])
    rot[0] = np.eye(n_out, n_in)
    trans = rng.uniform(-0.08, 0.08, size=(B, n_out))
    trans[0] = 0
    return rot, trans


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out, B=3):
    """The inputs (fp64 numpy) and the fp64 reference results, computed once and shared; never modified."""
    rng = np.random.default_rng(100 * n_in + n_out)
    grid = GRIDS[n_out]
    uni = rng.uniform(-1.15, 1.15, size=(20_000, n_in))
    uni = uni[~(uni[:, 0] >= 0.7)]
    centre = np.array([-0.31, 0.12, 0.05])[:n_in]
    packed = centre + rng.uniform(-0.2, 0.2, size=(2000, n_in)) / max(grid)
    corners = np.zeros((2 ** n_out, n_in))
    for k, s in enumerate(itertools.product((-1, 1), repeat=n_out)):
        corners[k, :n_out] = [sd * (1 - 1.0 / n) for sd, n in zip(s, grid)]
    pts = np.concatenate([uni, packed, corners])
    rot, trans = _poses(rng, B, n_in, n_out)
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, bg=rng.normal(size=B), ow=rng.uniform(0.5, 1.5, size=B),
             pw=rng.uniform(0.5, 1.5, size=len(pts)), g=rng.normal(size=grid + (B,)))
    c["out"] = SR.raster_smooth(grid, pts, rot, trans, c["bg"], c["ow"], c["pw"])
    c["out_default"] = SR.raster_smooth(grid, pts, rot, trans)
    c["pb"] = SR.raster_pullback_smooth(c["g"], pts, rot, trans, c["ow"], c["pw"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dev_args(c, dev, npdt, B, optional=True):
    a = [T(c["points"].astype(npdt), dev), T(c["rot"][:B].astype(npdt), dev), T(c["trans"][:B].astype(npdt), dev)]
    if optional:
        a += [T(c["bg"][:B].astype(npdt), dev), T(c["ow"][:B].astype(npdt), dev), T(c["pw"].astype(npdt), dev)]
    return a


def _check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    # the case does reach the branches it is built for (pose 0)
    assert c["out_default"][..., 0].sum() < len(c["points"]) - 100          # rejected points and dropped cells
    for B in (1, 3):
        out = dpr_amd.raster_smooth(c["grid"], *_dev_args(c, dev, npdt, B), algo=algo)
        assert out.shape == c["grid"] + (B,) and out.dtype == tdt
        assert_close(out, c["out"][..., :B].astype(npdt), tol(npdt, "out"), f"{algo} B={B}")
    out = dpr_amd.raster_smooth(c["grid"], *_dev_args(c, dev, npdt, 3, optional=False), algo=algo)
    assert_close(out, c["out_default"].astype(npdt), tol(npdt, "out"), f"{algo} defaults")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_equals_atomic(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    args = _dev_args(c, dev, npdt, 3)
    a = dpr_amd.raster_smooth(c["grid"], *args, algo="atomic")
    t = dpr_amd.raster_smooth(c["grid"], *args, algo="tiled")
    assert_close(t, a.cpu().numpy(), tol(npdt, "out"), "tiled vs atomic")
    # AUTO is one of the two
    assert dpr_amd.resolve_algo_smooth("raster", c["grid"], len(c["points"]), 3, n_in) in ("atomic", "tiled")
    auto = dpr_amd.raster_smooth(c["grid"], *args)
    assert_close(auto, a.cpu().numpy(), tol(npdt, "out"), "auto vs atomic")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_forward_of_a_permuted_cloud(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    perm = np.random.default_rng(9).permutation(len(c["points"]))
    pts, rot, trans, bg, ow, pw = _dev_args(c, dev, npdt, 3)
    assert float(pw.min()) > 0
    p = torch.as_tensor(perm, device=dev)
    a = dpr_amd.raster_smooth(c["grid"], pts, rot, trans, bg, ow, pw, algo="tiled")
    b = dpr_amd.raster_smooth(c["grid"], pts[p].contiguous(), rot, trans, bg, ow, pw[p].contiguous(), algo="tiled")
    assert_close(b, a.cpu().numpy(), tol(npdt, "out"), "permuted cloud")
    assert_close(b, c["out"].astype(npdt), tol(npdt, "out"), "permuted cloud vs reference")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_and_one_point(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    rot, trans, bg = T(c["rot"].astype(npdt), dev), T(c["trans"].astype(npdt), dev), T(c["bg"].astype(npdt), dev)
    out = dpr_amd.raster_smooth(c["grid"], torch.zeros((0, n_in), dtype=tdt, device=dev), rot, trans, bg, algo=algo)
    want = np.broadcast_to(c["bg"].astype(npdt), c["grid"] + (3,))
    assert np.array_equal(out.cpu().numpy(), want)
    one = np.full((1, n_in), 0.21)
    out = dpr_amd.raster_smooth(c["grid"], T(one.astype(npdt), dev), rot, trans, bg, algo=algo)
    assert_close(out, SR.raster_smooth(c["grid"], one, c["rot"], c["trans"], c["bg"]).astype(npdt), tol(npdt, "out"))


@pytest.mark.parametrize("algo", ["atomic", "tiled", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_known_answers(dev, algo, npdt, tdt):
    """5 x 5 grid, identity pose, one unit point (single-pose API)."""
    R, t = torch.eye(2, dtype=tdt, device=dev), torch.zeros(2, dtype=tdt, device=dev)
    k = np.array([1 / 8, 3 / 4, 1 / 8])
    out = dpr_amd.raster_smooth((5, 5), torch.zeros((1, 2), dtype=tdt, device=dev), R, t, algo=algo)
    assert out.shape == (5, 5) and out.dtype == tdt
    want = np.zeros((5, 5))
    want[1:4, 1:4] = np.outer(k, k)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=4 * np.finfo(npdt).eps)
    # (-1, 0): coord_x = 0, x-weights [1/2, 1/2, 0] with cell -1 dropped
    out = dpr_amd.raster_smooth((5, 5), torch.tensor([[-1.0, 0.0]], dtype=tdt, device=dev), R, t, algo=algo)
    want = np.zeros((5, 5))
    want[0, 1:4] = 0.5 * k
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=4 * np.finfo(npdt).eps)
    assert abs(float(out.sum()) - 0.5) <= 8 * np.finfo(npdt).eps


# ------------------------------------------------------------------ pullback
@pytest.mark.parametrize("algo", ["atomic", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    assert dpr_amd.resolve_algo_smooth("pullback", c["grid"], len(c["points"]), 3, n_in) == "atomic"
    g = grid_to_dev(c["g"].astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_(g, *_dev_args(c, dev, npdt, 3), algo=algo)
    assert pb.points.dtype == tdt and pb.rotation.shape == (3, n_out, n_in)
    _check_pullback(pb, c["pb"], npdt, "B=3 ")
    # B = 1: the gradients of pose 0 alone
    ref1 = SR.raster_pullback_smooth(c["g"][..., :1], c["points"], c["rot"][:1], c["trans"][:1], c["ow"][:1], c["pw"])
    pb1 = dpr_amd.raster_pullback_smooth_(grid_to_dev(c["g"][..., :1].astype(npdt), dev),
                                          *_dev_args(c, dev, npdt, 1), algo=algo)
    _check_pullback(pb1, ref1, npdt, "B=1 ")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_pullback_smooth_(g, *_dev_args(c, dev, npdt, 3), algo="tiled")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_of_many_poses_of_a_small_cloud(dev, npdt, tdt, n_in, n_out):
    """B = 70, P = 300 on an 8^N grid: the launch cuts the poses into slices (two blocks of points)."""
    rng = np.random.default_rng(7)
    B, P, grid = 70, 300, (8,) * n_out
    pts = rng.uniform(-1.15, 1.15, size=(P, n_in))
    rot, trans = _poses(rng, B, n_in, n_out)
    bg, ow, pw = rng.normal(size=B), rng.uniform(0.5, 1.5, size=B), rng.uniform(0.5, 1.5, size=P)
    g = rng.normal(size=grid + (B,))
    ref = SR.raster_pullback_smooth(g, pts, rot, trans, ow, pw)
    a = [T(x.astype(npdt), dev) for x in (pts, rot, trans, bg, ow, pw)]
    pb = dpr_amd.raster_pullback_smooth_(grid_to_dev(g.astype(npdt), dev), *a)
    _check_pullback(pb, ref, npdt, "B=70 ")
    out = dpr_amd.raster_smooth(grid, *a)
    assert_close(out, SR.raster_smooth(grid, pts, rot, trans, bg, ow, pw).astype(npdt), tol(npdt, "out"), "B=70 out")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_pullback_output_buffers_and_point_weight_grad(dev, npdt, tdt):
    n_in, n_out, B = 3, 3, 3
    c = _case(n_in, n_out)
    P = len(c["points"])
    g = grid_to_dev(c["g"].astype(npdt), dev)
    args = _dev_args(c, dev, npdt, B)
    # pre-allocated outputs are overwritten and returned by identity
    junk = lambda *s: torch.full(s, 7.5, dtype=tdt, device=dev)
    d_pts, d_rot_cm, d_tr = junk(P, n_in), junk(B, n_in, n_out), junk(B, n_out)
    d_bg, d_ow, d_pw = junk(B), junk(B), junk(P)
    pb = dpr_amd.raster_pullback_smooth_(g, *args, ds_dpoints=d_pts, ds_drotation=d_rot_cm.transpose(1, 2),
                                         ds_dtranslation=d_tr, ds_dbackground=d_bg, ds_dout_weight=d_ow,
                                         ds_dpoint_weight=d_pw)
    assert pb.points is d_pts and pb.translation is d_tr and pb.background is d_bg
    assert pb.out_weight is d_ow and pb.point_weight is d_pw
    assert pb.rotation.data_ptr() == d_rot_cm.data_ptr()
    _check_pullback(pb, c["pb"], npdt, "buffers ")
    # point_weight_grad=False: None comes back and nothing else changes
    nb = dpr_amd.raster_pullback_smooth_(g, *args, point_weight_grad=False)
    assert nb.point_weight is None
    _check_pullback(nb[:5], c["pb"][:5], npdt, "no pw grad ")
    with pytest.raises(ValueError):
        dpr_amd.raster_pullback_smooth_(g, *args, point_weight_grad=False, ds_dpoint_weight=d_pw)
    # ... and the C entry point leaves a ds_dpoint_weight buffer it is handed with the flag unwritten
    keep = junk(P)
    L = _lib.lib()
    grid = np.asarray(c["grid"], dtype=np.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pts, rot, trans, _bg, ow, pw = args
    rot_cm = rot.transpose(1, 2).contiguous()
    fn = getattr(L, "dpr_raster_pullback_smooth_ex_" + ("f32" if npdt == np.float32 else "f64"))
    rc = fn(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _lib.ALGO_ATOMIC,
            _lib.FLAG_NO_POINT_WEIGHT_GRAD, n_in, n_out, grid.ctypes.data_as(ctypes.c_void_p), P, B, p(g), p(pts),
            p(rot_cm), p(trans), p(ow), p(pw), p(d_pts), p(d_rot_cm), p(d_tr), p(d_bg), p(d_ow), p(keep), None, 0)
    torch.cuda.synchronize()
    assert rc == _lib.OK, _lib.last_error()
    assert bool((keep == 7.5).all())
    assert_close(d_pts, c["pb"][0].astype(npdt), tol(npdt, "points"), "flagged C call, ds_dpoints")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_of_an_empty_cloud_with_several_poses(dev, npdt, tdt, n_in, n_out):
    """P = 0, B = 3: the point gradients are empty, the per-pose sums exactly 0, ds_dbackground the plane sums; and
    the backward of raster_smooth_ad on an empty cloud with two poses.  (The pose slicing of the launch divides by
    the number of point blocks: before the pullback returned ahead of it, this call ended the process.)"""
    c = _case(n_in, n_out)
    B = 3
    g = c["g"].astype(npdt)
    rot, trans, bg, ow = (T(c[k][:B].astype(npdt), dev) for k in ("rot", "trans", "bg", "ow"))
    none = torch.zeros((0, n_in), dtype=tdt, device=dev)
    pb = dpr_amd.raster_pullback_smooth_(grid_to_dev(g, dev), none, rot, trans, bg, ow,
                                         torch.zeros(0, dtype=tdt, device=dev))
    assert tuple(pb.points.shape) == (0, n_in) and tuple(pb.point_weight.shape) == (0,)
    assert pb.points.dtype == tdt and pb.point_weight.dtype == tdt
    assert tuple(pb.rotation.shape) == (B, n_out, n_in) and tuple(pb.translation.shape) == (B, n_out)
    for f in ("rotation", "translation", "out_weight"):
        assert not bool((getattr(pb, f) != 0).any()), f"ds_d{f} of an empty cloud is not 0"
    assert tuple(pb.background.shape) == (B,)
    assert_close(pb.background, g.astype(np.float64).reshape(-1, B).sum(axis=0).astype(npdt), tol(npdt, "pose"),
                 "ds_dbackground")
    # autograd: two poses, no point
    xs = [none.clone().requires_grad_(True)] + [x[:2].clone().requires_grad_(True) for x in (rot, trans, bg, ow)]
    for algo in ("atomic", "tiled"):
        for x in xs:
            x.grad = None
        out = dpr_amd.raster_smooth_ad(c["grid"], *xs, algo=algo)
        assert tuple(out.shape) == c["grid"] + (2,)
        w = grid_to_dev(g[..., :2], dev)
        (out * w).sum().backward()
        assert tuple(xs[0].grad.shape) == (0, n_in)
        assert not bool((xs[1].grad != 0).any()) and not bool((xs[2].grad != 0).any())
        assert not bool((xs[4].grad != 0).any())
        assert_close(xs[3].grad, g[..., :2].astype(np.float64).reshape(-1, 2).sum(axis=0).astype(npdt),
                     tol(npdt, "pose"), f"{algo}: background.grad")


# ------------------------------------------------------------------ derivative tests on the device
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, n_in, n_out):
    """raster_smooth_ad in fp64 on an 8^N grid with 10 points (the reference's test/chainrules.jl shape): central
    differences with h = 1e-6 of sum(out * g) in all six arguments, within 1e-6 * max|gradient| (the bound of
    tests/test_smooth_reference.py: truncation h^2 and rounding eps / h are both ~1e-10 relative)."""
    rng = np.random.default_rng(11)
    B, P, grid = 2, 10, (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(P, n_in)), rot, trans, rng.normal(size=B), rng.uniform(0.5, 1.5, size=B),
            rng.uniform(0.5, 1.5, size=P)]
    g = grid_to_dev(rng.normal(size=grid + (B,)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    out = dpr_amd.raster_smooth_ad(grid, *xs)
    (out * g).sum().backward()
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
                up = float((dpr_amd.raster_smooth(grid, *xs) * g).sum())
                flat[i] = keep - h
                dn = float((dpr_amd.raster_smooth(grid, *xs) * g).sum())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (FIELDS[k], err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_gradient_is_continuous_across_a_cell_boundary(dev, n_in, n_out):
    """Points 1e-9 either side of an integer coord (fp64): the GPU pullback's gradients differ by less than
    1e-6 * max|gradient|, and agree with the reference on both sides."""
    rng = np.random.default_rng(5)
    grid = (8,) * n_out
    g = rng.normal(size=grid + (1,))
    rot, trans = np.eye(n_out, n_in)[None], np.zeros((1, n_out))
    base = rng.uniform(-0.5, 0.5, size=(6, n_in))
    base[:, 0] = -1 + 2.0 * np.array([2, 3, 4, 5, 6, 3]) / grid[0]
    lo, hi = base.copy(), base.copy()
    lo[:, 0] -= 1e-9 * 2 / grid[0]
    hi[:, 0] += 1e-9 * 2 / grid[0]
    assert np.all(np.floor((lo[:, 0] + 1) * 4) + 1 == np.floor((hi[:, 0] + 1) * 4))
    gd = grid_to_dev(g, dev)
    run = lambda p: dpr_amd.raster_pullback_smooth_(gd, T(p, dev), T(rot, dev), T(trans, dev))
    pa, pb = run(lo), run(hi)
    scale = max(float(a.abs().max()) for a in pa)
    assert float((pa.points - pb.points).abs().max()) < 1e-6 * scale
    assert float((pa.point_weight - pb.point_weight).abs().max()) < 1e-6 * scale
    _check_pullback(pa, SR.raster_pullback_smooth(g, lo, rot, trans), np.float64, "low side ")
    _check_pullback(pb, SR.raster_pullback_smooth(g, hi, rot, trans), np.float64, "high side ")


# ------------------------------------------------------------------ batch vs single pose
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_pose_alone_equals_its_plane_and_rows_in_a_batch(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    pts, rot, trans, bg, ow, pw = _dev_args(c, dev, npdt, 3)
    g = grid_to_dev(c["g"].astype(npdt), dev)
    out = dpr_amd.raster_smooth(c["grid"], pts, rot, trans, bg, ow, pw, algo="tiled")
    pb = dpr_amd.raster_pullback_smooth_(g, pts, rot, trans, bg, ow, pw)
    b = 1
    single = (pts, rot[b], trans[b], float(bg[b]), float(ow[b]), pw)
    for algo in ("atomic", "tiled"):
        o1 = dpr_amd.raster_smooth(c["grid"], *single, algo=algo)
        assert o1.shape == c["grid"]
        assert_close(o1, out[..., b].cpu().numpy(), tol(npdt, "out"), f"single pose, {algo}")
    g1 = dpr_amd.to_grid_layout(g[..., b])
    p1 = dpr_amd.raster_pullback_smooth_(g1, *single)
    assert p1.rotation.shape == (n_out, n_in) and p1.translation.shape == (n_out,)
    assert p1.background.ndim == 0 and p1.out_weight.ndim == 0
    for name, a, e in (("rotation", p1.rotation, pb.rotation[b]), ("translation", p1.translation, pb.translation[b]),
                       ("background", p1.background, pb.background[b]),
                       ("out_weight", p1.out_weight, pb.out_weight[b])):
        assert_close(a, e.cpu().numpy(), tol(npdt, "pose"), f"single pose {name}")
    ref1 = SR.raster_pullback_smooth(c["g"][..., b:b + 1], c["points"], c["rot"][b:b + 1], c["trans"][b:b + 1],
                                     c["ow"][b:b + 1], c["pw"])
    assert_close(p1.points, ref1[0].astype(npdt), tol(npdt, "points"), "single pose points")
    assert_close(p1.point_weight, ref1[5].astype(npdt), tol(npdt, "points"), "single pose point_weight")
    # one pose: one thread adds a point's terms and stores once -- the same bits on every run
    p2 = dpr_amd.raster_pullback_smooth_(g1, *single)
    assert torch.equal(p1.points, p2.points) and torch.equal(p1.point_weight, p2.point_weight)
