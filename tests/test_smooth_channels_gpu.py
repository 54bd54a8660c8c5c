"""The smooth splat with C weights per point on the GPU (dpr_amd.raster_smooth_channels / raster_pullback_smooth_channels_
/ raster_smooth_channels_ad) against the numpy reference tests/smooth_channels_reference.py evaluated in fp64.
Tolerances: the project's norm-wise ones (tests/test_parity_gpu.py: fp64 1e-10; fp32 5e-5 `out`, 1e-4 point
gradients, 1e-3 pose gradients).

The case is that of tests/test_smooth_gpu.py, built here: grids with three tiles and a partial last tile on every
axis of the tiled forward's tiles ((37, 19, 21), (150, 37)); 20 000 points uniform in +-1.15 with the slab
0.7 <= x_0 left empty, 2 000 points packed into one cell, one point at the centre of each corner cell; three poses,
pose 0 the identity.  Sixteen weight channels: channel 1 is all zero, channel 2 has both signs.  C = 1, 3, 5, 16 are
the first C of them: 3 and 5 end in a half-filled chunk of the tiled forward's 2 channels per workgroup, 5 crosses the
small bound of 4 channels of the atomic forward and of the pullback and takes their 16-channel kernels, 16 is the
bound.  The fp64 reference is computed once per (N_in, N_out), channel by channel, and shared."""
import functools
import itertools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_channels_reference as SCR
from tests import smooth_reference as SR
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (150, 37), 3: (37, 19, 21)}
CHANNELS = [1, 3, 5, 16]
CMAX = 16
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


def _weights(rng, P, C=CMAX):
    pw = rng.uniform(0.5, 1.5, size=(P, C))
    if C > 1:
        pw[:, 1] = 0.0
    if C > 2:
        pw[:, 2] = rng.uniform(-1.0, 1.0, size=P)
    return pw


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out, B=3):
    """The inputs (fp64 numpy) and the fp64 reference results for 16 channels, computed once and shared; never
    modified.  `unit`: the planes for background 0 and out_weight 1; `parts`: the gradients channel by channel;
    `parts1`: those of pose 0 alone."""
    rng = np.random.default_rng(200 * n_in + n_out)
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
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, bg=rng.normal(size=(B, CMAX)),
             ow=rng.uniform(0.5, 1.5, size=B), pw=_weights(rng, len(pts)), g=rng.normal(size=grid + (CMAX, B)))
    c["unit"] = SCR.raster_smooth_channels(grid, pts, rot, trans, c["pw"])
    c["parts"] = SCR.pullback_parts(c["g"], pts, rot, trans, c["pw"], c["ow"])
    c["parts1"] = SCR.pullback_parts(c["g"][..., :1], pts, rot[:1], trans[:1], c["pw"], c["ow"][:1])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _out_ref(c, C, B, optional=True):
    """grid + (C, B): background + out_weight * the unit planes (the reference is linear in both)."""
    unit = c["unit"][..., :C, :B]
    return c["bg"][:B, :C].T + c["ow"][:B] * unit if optional else unit


def _dev_args(c, dev, npdt, C, B, optional=True):
    """points, rotation, translation, point_weight[, background, out_weight]"""
    a = [T(c["points"].astype(npdt), dev), T(c["rot"][:B].astype(npdt), dev), T(c["trans"][:B].astype(npdt), dev),
         T(c["pw"][:, :C].astype(npdt), dev)]
    if optional:
        a += [T(c["bg"][:B, :C].astype(npdt), dev), T(c["ow"][:B].astype(npdt), dev)]
    return a


def _grads(pb):
    return (pb.points, pb.rotation, pb.translation, pb.background, pb.out_weight, pb.point_weight)


def _check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, _grads(pb), ref):
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("algo", ["atomic", "tiled", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out, C):
    c = _case(n_in, n_out)
    # the case does reach the branches it is built for (pose 0, channel 0)
    assert c["unit"][..., 0, 0].sum() < c["pw"][:, 0].sum() - 100          # rejected points and dropped cells
    if C >= 3:
        assert not c["unit"][..., 1, :].any() and c["unit"][..., 2, :].min() < 0 < c["unit"][..., 2, :].max()
    for B in (1, 3):
        out = dpr_amd.raster_smooth_channels(c["grid"], *_dev_args(c, dev, npdt, C, B), algo=algo)
        assert out.shape == c["grid"] + (C, B) and out.dtype == tdt
        assert_close(out, _out_ref(c, C, B).astype(npdt), tol(npdt, "out"), f"{algo} C={C} B={B}")
        for ch in range(C):  # plane by plane: a channel of small norm is held to its own norm
            assert_close(out[..., ch, :], _out_ref(c, C, B)[..., ch, :].astype(npdt), tol(npdt, "out"),
                         f"{algo} C={C} B={B} channel {ch}")
    out = dpr_amd.raster_smooth_channels(c["grid"], *_dev_args(c, dev, npdt, C, 3, optional=False), algo=algo)
    assert_close(out, _out_ref(c, C, 3, optional=False).astype(npdt), tol(npdt, "out"), f"{algo} C={C} defaults")
    if C >= 3:  # a channel of zero weights on a zero background stays exactly zero
        assert not bool(out[..., 1, :].any())


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_equals_atomic_and_a_permuted_cloud(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    C = 5
    pts, rot, trans, pw, bg, ow = _dev_args(c, dev, npdt, C, 3)
    a = dpr_amd.raster_smooth_channels(c["grid"], pts, rot, trans, pw, bg, ow, algo="atomic")
    t = dpr_amd.raster_smooth_channels(c["grid"], pts, rot, trans, pw, bg, ow, algo="tiled")
    assert_close(t, a.cpu().numpy(), tol(npdt, "out"), "tiled vs atomic")
    assert dpr_amd.resolve_algo_smooth_channels("raster", c["grid"], len(c["points"]), 3, n_in, C) in ("atomic",
                                                                                                        "tiled")
    p = torch.as_tensor(np.random.default_rng(9).permutation(len(c["points"])), device=dev)
    b = dpr_amd.raster_smooth_channels(c["grid"], pts[p].contiguous(), rot, trans, pw[p].contiguous(), bg, ow,
                                       algo="tiled")
    assert_close(b, t.cpu().numpy(), tol(npdt, "out"), "permuted cloud")
    assert_close(b, _out_ref(c, C, 3).astype(npdt), tol(npdt, "out"), "permuted cloud vs reference")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_plane_is_raster_smooth_of_its_channel(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    C = 3
    pts, rot, trans, pw, bg, ow = _dev_args(c, dev, npdt, C, 3)
    out = dpr_amd.raster_smooth_channels(c["grid"], pts, rot, trans, pw, bg, ow, algo=algo)
    for ch in range(C):
        one = dpr_amd.raster_smooth(c["grid"], pts, rot, trans, bg[:, ch].contiguous(), ow, pw[:, ch].contiguous(),
                                    algo=algo)
        assert_close(out[..., ch, :], one.cpu().numpy(), tol(npdt, "out"), f"{algo} channel {ch}")


# ------------------------------------------------------------------ pullback
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_matches_the_reference(dev, npdt, tdt, n_in, n_out, C):
    c = _case(n_in, n_out)
    B, P = 3, len(c["points"])
    pts, rot, trans, pw, bg, ow = _dev_args(c, dev, npdt, C, B)
    g = grid_to_dev(c["g"][..., :C, :].astype(npdt), dev)
    ref = SCR.combine(c["parts"][:C])
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[5][:, 0]).max() > 0
    for algo in ("atomic", "auto"):
        pb = dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, bg, ow, algo=algo)
        assert pb.point_weight.shape == (P, C) and pb.background.shape == (B, C)
        _check_pullback(pb, ref, npdt, f"{algo} C={C} ")
        for ch in range(C):  # per channel: a channel's own norm
            assert_close(pb.point_weight[:, ch], ref[5][:, ch].astype(npdt), tol(npdt, "points"),
                         f"ds_dpoint_weight[:, {ch}]")
    # keyword buffers: returned by identity, every element overwritten
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device=dev)
    bufs = dict(ds_dpoints=nan(P, n_in), ds_drotation=nan(B, n_in, n_out).transpose(-1, -2), ds_dtranslation=nan(B, n_out),
                ds_dbackground=nan(B, C), ds_dout_weight=nan(B), ds_dpoint_weight=nan(P, C))
    pb = dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, bg, ow, **bufs)
    for name, got in zip(FIELDS, _grads(pb)):
        if name == "rotation":  # (handed in as the transposed view of the column-major buffer: the same memory)
            assert got.data_ptr() == bufs["ds_drotation"].data_ptr() and got.shape == (B, n_out, n_in)
        else:
            assert got is bufs["ds_d" + name], name
        assert bool(torch.isfinite(got).all()), name
    _check_pullback(pb, ref, npdt, "buffers ")
    # without the point-weight gradient
    pb = dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, bg, ow, point_weight_grad=False)
    assert pb.point_weight is None
    for name, kind, a, e in list(zip(FIELDS, KINDS, _grads(pb), ref))[:5]:
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"point_weight_grad=False {name}")
    with pytest.raises(ValueError):
        dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, point_weight_grad=False,
                                                 ds_dpoint_weight=bufs["ds_dpoint_weight"])


@pytest.mark.parametrize("C", [3, 5, 16])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_of_one_pose_matches_the_reference(dev, npdt, tdt, n_in, n_out, C):
    """One pose is one pose slice: ds_dpoints and ds_dpoint_weight (P, C) leave the kernel as plain stores, not as the
    atomics onto zeroed buffers that every batch of this file takes (B > 1 and fewer than 524 033 points are sliced).
    C = 3 on the 4-channel kernel, 5 and 16 on the 16-channel one.  Batched (B = 1) and single-pose arguments, the
    latter with a ColumnMajorRotation and a (C,) background; include/dpr.h promises the stored gradients of one slice
    bit-reproducible, so the two calls give the same bits."""
    c = _case(n_in, n_out)
    P = len(c["points"])
    pts, rot, trans, pw, bg, ow = _dev_args(c, dev, npdt, C, 1)
    g = grid_to_dev(c["g"][..., :C, :1].astype(npdt), dev)
    ref = SCR.combine(c["parts1"][:C])
    pb = dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, bg, ow)
    assert pb.point_weight.shape == (P, C) and pb.background.shape == (1, C)
    _check_pullback(pb, ref, npdt, f"B=1 C={C} ")
    for ch in range(C):
        assert_close(pb.point_weight[:, ch], ref[5][:, ch].astype(npdt), tol(npdt, "points"),
                     f"ds_dpoint_weight[:, {ch}]")
    one = dpr_amd.raster_pullback_smooth_channels_(g[..., 0], pts, dpr_amd.column_major_rotation(rot[0]), trans[0], pw,
                                                   bg[0], ow[0])
    assert one.rotation.shape == (n_out, n_in) and one.background.shape == (C,)
    assert torch.equal(one.points, pb.points) and torch.equal(one.point_weight, pb.point_weight)
    for name, kind, a, e in list(zip(FIELDS, KINDS, _grads(one), ref))[1:5]:
        assert_close(a, e[0].astype(npdt), tol(npdt, kind), f"single pose {name}")
    # the forward takes the same arguments
    out = dpr_amd.raster_smooth_channels(c["grid"], pts, dpr_amd.column_major_rotation(rot[0]), trans[0], pw, bg[0],
                                         ow[0])
    assert out.shape == c["grid"] + (C,)
    assert_close(out, _out_ref(c, C, 1)[..., 0].astype(npdt), tol(npdt, "out"), "single pose forward")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_one_channel_is_the_smooth_pullback(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    for B in (1, 3):
        pts, rot, trans, pw, bg, ow = _dev_args(c, dev, npdt, 1, B)
        g = grid_to_dev(c["g"][..., :1, :B].astype(npdt), dev)
        pb = dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, bg, ow)
        one = dpr_amd.raster_pullback_smooth_(g[..., 0, :], pts, rot, trans, bg[:, 0].contiguous(), ow,
                                              pw[:, 0].contiguous())
        want = (one.points, one.rotation, one.translation, one.background[:, None], one.out_weight,
                one.point_weight[:, None])
        for name, kind, a, e in zip(FIELDS, KINDS, _grads(pb), want):
            assert_close(a, e.cpu().numpy(), tol(npdt, kind), f"B={B} {name}")


def test_the_pullback_has_no_tiled_path(dev):
    c = _case(3, 3)
    pts, rot, trans, pw = _dev_args(c, dev, np.float32, 3, 3, optional=False)
    g = grid_to_dev(c["g"][..., :3, :].astype(np.float32), dev)
    with pytest.raises(dpr_amd.DprError, match="DPR_ALGO_ATOMIC only"):
        dpr_amd.raster_pullback_smooth_channels_(g, pts, rot, trans, pw, algo="tiled")


# ------------------------------------------------------------------ autograd
def test_autograd_matches_differences_and_the_direct_pullback(dev):
    """fp64, grid (9, 7, 8), 40 points, C = 3, B = 2: d<out, g> along a random direction of all six inputs by central
    differences (h = 1e-6; the operator is C1 and the random points sit away from cell faces by far more than h, so
    the truncation is O(h^2) and the bound 1e-7 of the gradient's norm is generous) against autograd, and autograd's
    gradients against the direct pullback call."""
    grid, P, C, B = (9, 7, 8), 40, 3, 2
    rng = np.random.default_rng(77)
    pts = rng.uniform(-1.1, 1.1, size=(P, 3))
    rot, trans = _poses(rng, B, 3, 3)
    pw, bg, ow = _weights(rng, P, C), rng.normal(size=(B, C)), rng.uniform(0.5, 1.5, size=B)
    g = grid_to_dev(rng.normal(size=grid + (C, B)), dev)
    host = [pts, rot, trans, pw, bg, ow]
    args = [T(a, dev).requires_grad_(True) for a in host]
    for algo in ("auto", "atomic", "tiled"):
        out = dpr_amd.raster_smooth_channels_ad(grid, *args, algo=algo)
        grads = torch.autograd.grad((out * g).sum(), args)
        pb = dpr_amd.raster_pullback_smooth_channels_(g, *[a.detach() for a in args])
        direct = (pb.points, pb.rotation, pb.translation, pb.point_weight, pb.background, pb.out_weight)
        for name, a, e in zip(("points", "rotation", "translation", "point_weight", "background", "out_weight"),
                              grads, direct):
            assert_close(a, e.cpu().numpy(), 1e-12, f"{algo} autograd vs pullback: {name}")
    dirs = [rng.normal(size=a.shape) for a in host]
    h = 1e-6
    loss = lambda s: float((dpr_amd.raster_smooth_channels(grid, *[T(a + s * h * d, dev) for a, d in zip(host, dirs)],
                                                           algo="atomic") * g).sum())
    fd = (loss(1.0) - loss(-1.0)) / (2 * h)
    an = sum(float((gr.cpu().numpy() * d).sum()) for gr, d in zip(grads, dirs))
    scale = np.sqrt(sum(float((gr ** 2).sum()) for gr in grads)) * np.sqrt(sum((d ** 2).sum() for d in dirs))
    assert abs(fd - an) <= 1e-7 * scale, (fd, an, scale)
    # only the inputs that ask get a gradient
    only = [T(a, dev) for a in host]
    only[3].requires_grad_(True)
    out = dpr_amd.raster_smooth_channels_ad(grid, *only)
    (gpw,) = torch.autograd.grad((out * g).sum(), [only[3]])
    assert_close(gpw, direct[3].cpu().numpy(), 1e-12, "point_weight alone")


# ------------------------------------------------------------------ edge sizes
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_edge_sizes(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    C, B, grid = 5, 3, c["grid"]
    rot, trans = T(c["rot"].astype(npdt), dev), T(c["trans"].astype(npdt), dev)
    bg = T(c["bg"][:, :C].astype(npdt), dev)
    bg_planes = np.broadcast_to(c["bg"][:, :C].T.astype(npdt), grid + (C, B))
    g = grid_to_dev(c["g"][..., :C, :].astype(npdt), dev)
    g_sums = c["g"][..., :C, :].astype(npdt).reshape(-1, C, B).sum(axis=0, dtype=np.float64).T
    empty = lambda *shape: torch.zeros(shape, dtype=tdt, device=dev)
    # P = 0: the backgrounds; the gradients 0, ds_dbackground the plane sums
    out = dpr_amd.raster_smooth_channels(grid, empty(0, n_in), rot, trans, empty(0, C), bg, algo=algo)
    assert np.array_equal(out.cpu().numpy(), bg_planes)
    pb = dpr_amd.raster_pullback_smooth_channels_(g, empty(0, n_in), rot, trans, empty(0, C))
    assert pb.points.shape == (0, n_in) and pb.point_weight.shape == (0, C)
    assert not bool(pb.rotation.any()) and not bool(pb.translation.any()) and not bool(pb.out_weight.any())
    assert_close(pb.background, g_sums.astype(npdt), tol(npdt, "pose"), "P = 0 ds_dbackground")
    # B = 0
    pts = T(c["points"][:100].astype(npdt), dev)
    pw = T(c["pw"][:100, :C].astype(npdt), dev)
    out = dpr_amd.raster_smooth_channels(grid, pts, empty(0, n_out, n_in), empty(0, n_out), pw, algo=algo)
    assert out.shape == grid + (C, 0)
    pb = dpr_amd.raster_pullback_smooth_channels_(dpr_amd.empty_channel_grid(grid, C, 0, tdt, dev), pts,
                                                  empty(0, n_out, n_in), empty(0, n_out), pw)
    assert pb.rotation.shape == (0, n_out, n_in) and pb.background.shape == (0, C)
    # P = 1
    one = np.full((1, n_in), 0.21)
    w1 = c["pw"][:1, :C]
    out = dpr_amd.raster_smooth_channels(grid, T(one.astype(npdt), dev), rot, trans, T(w1.astype(npdt), dev), bg,
                                         algo=algo)
    want = SCR.raster_smooth_channels(grid, one, c["rot"], c["trans"], w1, c["bg"][:, :C])
    assert_close(out, want.astype(npdt), tol(npdt, "out"), "P = 1")
    pb = dpr_amd.raster_pullback_smooth_channels_(g, T(one.astype(npdt), dev), rot, trans, T(w1.astype(npdt), dev))
    _check_pullback(pb, SCR.raster_pullback_smooth_channels(c["g"][..., :C, :], one, c["rot"], c["trans"], w1), npdt,
                    "P = 1 ")
    # a cloud wholly outside the grid (identity poses, every coordinate beyond 1.8): every plane is its background,
    # the point gradients are 0
    far = T((3.0 + c["points"][:500]).astype(npdt), dev)
    wf = T(c["pw"][:500, :C].astype(npdt), dev)
    rot = T(np.broadcast_to(np.eye(n_out, n_in), (B, n_out, n_in)).astype(npdt), dev)
    trans = torch.zeros_like(trans)
    out = dpr_amd.raster_smooth_channels(grid, far, rot, trans, wf, bg, algo=algo)
    assert np.array_equal(out.cpu().numpy(), bg_planes)
    pb = dpr_amd.raster_pullback_smooth_channels_(g, far, rot, trans, wf)
    assert not bool(pb.points.any()) and not bool(pb.point_weight.any()) and not bool(pb.rotation.any())


# ------------------------------------------------------------------ launch cuts and offsets past 2^32
def test_planes_across_the_launch_cut(dev):
    """Grid (8, 8), 300 points, C = 16, B = 4100: 65 600 planes, more than the 65 535 of one launch of the background
    fill and of the plane sums, and 4100 poses on the pose slices of the pullback.  Poses 0, 4095 (its planes
    65 520 .. 65 535 straddle the cut) and 4099, channels 0, 2 and 15, forward and pullback; every other output is
    held to being finite."""
    grid, P, C, B = (8, 8), 300, 16, 4100
    assert B * C > 65535 and 4095 * C < 65535 < 4096 * C
    rng = np.random.default_rng(5)
    r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pts = r32(rng.uniform(-1.1, 1.1, size=(P, 2)))
    ang = rng.uniform(0, 2 * np.pi, size=B)
    rot = r32(np.stack([np.stack([np.cos(ang), -np.sin(ang)], -1), np.stack([np.sin(ang), np.cos(ang)], -1)], -2))
    trans = r32(rng.uniform(-0.1, 0.1, size=(B, 2)))
    pw, bg, ow = r32(_weights(rng, P)), r32(rng.normal(size=(B, C))), r32(rng.uniform(0.5, 1.5, size=B))
    f32 = lambda a: T(np.asarray(a, np.float32), dev)
    poses, chans = [0, 4095, 4099], [0, 2, 15]
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_channels(grid, f32(pts), f32(rot), f32(trans), f32(pw), f32(bg), f32(ow), algo=algo)
        assert bool(torch.isfinite(out).all())
        for b in poses:
            want = SCR.raster_smooth_channels(grid, pts, rot[b:b + 1], trans[b:b + 1], pw[:, chans],
                                              bg[b:b + 1][:, chans], ow[b:b + 1])
            assert_close(out[..., chans, b], want[..., 0].astype(np.float32), tol(np.float32, "out"),
                         f"{algo} pose {b}")
    # the pullback: ds_dout is non-zero in the three poses only, so ds_dpoints is their sum
    gh = np.zeros(grid + (C, B), np.float32)
    gh[..., poses] = rng.normal(size=grid + (C, 3)).astype(np.float32)
    pb = dpr_amd.raster_pullback_smooth_channels_(grid_to_dev(gh, dev), f32(pts), f32(rot), f32(trans), f32(pw),
                                                  f32(bg), f32(ow))
    sel = list(poses)
    ref = SCR.raster_pullback_smooth_channels(gh[..., sel].astype(np.float64), pts, rot[sel], trans[sel], pw, ow[sel])
    assert_close(pb.points, ref[0].astype(np.float32), tol(np.float32, "points"), "ds_dpoints")
    assert_close(pb.point_weight, ref[5].astype(np.float32), tol(np.float32, "points"), "ds_dpoint_weight")
    for name, got, e in (("rotation", pb.rotation, ref[1]), ("translation", pb.translation, ref[2]),
                         ("background", pb.background, ref[3]), ("out_weight", pb.out_weight, ref[4])):
        assert_close(got[sel], e.astype(np.float32), tol(np.float32, "pose"), f"ds_d{name}")
        rest = np.ones(B, bool)
        rest[sel] = False
        assert not bool(got[torch.as_tensor(rest, device=dev)].any()), f"ds_d{name} of a pose without ds_dout"


def test_planes_past_2_pow_32(dev):
    """16 channels x 17 poses of 256^3 in fp32 (18 GB per image): planes 256 .. 271 are pose 16 and lie at or past
    element 2^32, the smallest size at which a 32-bit plane offset can show.  ATOMIC and TILED forward with out_weight
    zero except for poses 0 and 16: the first and the last plane against the reference, the poses between held to
    their backgrounds.  The pullback with ds_dout zero except in channels 0, 2 and 15 of pose 16 (the last plane of
    either chunk of eight channels among them): the point gradients, ds_dpoint_weight and the last pose's sums.  One
    plane at a time goes to the host."""
    grid, C, B, P = (256,) * 3, 16, 17, 1000
    G, last = 256 ** 3, B - 1
    assert last * C * G >= 2 ** 32
    free, _total = torch.cuda.mem_get_info(dev)
    assert free >= 2.5 * 4 * G * C * B, f"this test needs {2.5 * 4 * G * C * B / 2**30:.0f} GiB of free device memory"
    rng = np.random.default_rng(61)
    F32 = np.float32
    r64 = lambda a: np.asarray(a, np.float64)
    pts = (0.4 * rng.standard_normal(size=(P, 3))).astype(F32)
    q, _ = np.linalg.qr(rng.normal(size=(B, 3, 3)))
    R, t = q.astype(F32), (0.1 * rng.normal(size=(B, 3))).astype(F32)
    pw = _weights(rng, P).astype(F32)
    bg = ((np.arange(B * C) - B * C // 2) / 16.0).reshape(B, C).astype(F32)
    ow_all = rng.uniform(0.5, 1.5, size=B).astype(F32)
    ow = np.zeros_like(ow_all)
    ow[0], ow[last] = ow_all[0], ow_all[last]
    dpts, dR, dt, dpw, dbg = (T(a, dev) for a in (pts, R, t, pw, bg))
    planes = ((0, 0), (last, C - 1))
    refs = {(b, c): SR.raster_smooth(grid, r64(pts), r64(R[b:b + 1]), r64(t[b:b + 1]), r64(bg[b:b + 1, c]),
                                     r64(ow[b:b + 1]), r64(pw[:, c]))[..., 0].astype(F32) for b, c in planes}
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_channels(grid, dpts, dR, dt, dpw, dbg, T(ow, dev), algo=algo)
        torch.cuda.synchronize()
        for b, c in planes:
            got = out[..., c, b].cpu().numpy()
            assert_close(got, refs[(b, c)], tol(F32, "out"), f"{algo}: plane ({c}, {b})")
        mem = out.permute(4, 3, 2, 1, 0)
        assert mem.is_contiguous()
        for b in range(1, last):
            assert bool((mem[b] == dbg[b].reshape(C, 1, 1, 1)).all()), f"{algo}: pose {b} is not its background"
        del out, mem
        torch.cuda.empty_cache()
    del refs
    gen = torch.Generator(device=dev).manual_seed(61)
    g_mem = torch.zeros((B, C) + grid, dtype=torch.float32, device=dev)
    chans = (0, 2, C - 1)
    for c in chans:
        g_mem[last, c].normal_(generator=gen)
    g = g_mem.permute(4, 3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_smooth_channels_(g, dpts, dR, dt, dpw, dbg, T(ow_all, dev))
    torch.cuda.synchronize()
    parts = []
    for c in chans:
        plane = g[..., c, last].cpu().numpy()
        parts.append(SR.raster_pullback_smooth(r64(plane)[..., None], r64(pts), r64(R[last:]), r64(t[last:]),
                                               r64(ow_all[last:]), r64(pw[:, c])))
    ref = SCR.combine(parts)  # (the other channels of the pose have ds_dout = 0 and add nothing)
    sel = list(chans)
    assert_close(pb.points, ref[0].astype(F32), tol(F32, "points"), "ds_dpoints")
    assert_close(pb.point_weight[:, sel], ref[5].astype(F32), tol(F32, "points"), "ds_dpoint_weight")
    assert_close(pb.background[last:, sel], ref[3].astype(F32), tol(F32, "pose"), f"ds_dbackground[{last}]")
    rest = [c for c in range(C) if c not in chans]
    assert not bool(pb.point_weight[:, rest].any()) and not bool(pb.background[:, rest].any())
    for name, got, e in (("rotation", pb.rotation, ref[1]), ("translation", pb.translation, ref[2]),
                         ("out_weight", pb.out_weight, ref[4])):
        assert_close(got[last:], e.astype(F32), tol(F32, "pose"), f"ds_d{name}[{last}]")
    for name in ("rotation", "translation", "out_weight", "background"):
        assert not bool((getattr(pb, name)[:last] != 0).any()), f"ds_d{name} of the poses before the last is not 0"
    del g, g_mem, pb
    torch.cuda.empty_cache()
