"""The smooth splat of per-pose clouds on the GPU (dpr_amd.raster_smooth_clouds / raster_pullback_smooth_clouds_ /
raster_smooth_clouds_ad; include/dpr.h, SMOOTH SPLAT, PER-POSE CLOUDS) against the numpy reference
tests/smooth_reference.py, evaluated in fp64 pose by pose on (cloud b, pose b).  Tolerances: the project's norm-wise
ones (tests/test_parity_gpu.py: fp64 1e-10; fp32 5e-5 `out`, 1e-4 point gradients, 1e-3 pose gradients).

Shapes: the smallest that reach the hazards.  Grids (70, 20) and (20, 12, 9): 2 x 2 and 2 x 2 x 2 tiles of the tiled
forward (64 x 16, 16 x 8 x 8), a partial tile on every axis.  P = 300 (not a multiple of 256, two blocks), B = 5
(pose groups of 2 + 2 + 1 with max_pose_group=2).  Every cloud is drawn in the frame of its own pose so that its
coordinates span -2 .. n + 2 on every axis, with points planted at j0 = -1 and j0 = n of every axis (accepted, their
tile is that of the clamped cell), and rejected points."""
import ctypes
import functools

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
GRIDS = {2: (70, 20), 3: (20, 12, 9)}
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")
P, B = 300, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _poses(rng, nb, n_in, n_out):
    """Pose 0: the identity; the others: random rotations (rows of an orthogonal matrix) and small shifts."""
    q, _ = np.linalg.qr(rng.normal(size=(nb, n_in, n_in)))
    rot = np.ascontiguousarray(q[:, :n_out, :])
    rot[0] = np.eye(n_out, n_in)
    trans = rng.uniform(-0.08, 0.08, size=(nb, n_out))
    trans[0] = 0
    return rot, trans


def _coords(grid, pts, rot, trans):
    return ((pts @ rot.T + trans) + 1) * (np.asarray(grid) / 2)


def _cloud(rng, grid, rot, trans, n_in, n_points, lo=-2.0, hi=2.0, plant=False):
    """n_points points whose coord under (rot, trans) is uniform in [lo, n + hi) on every axis; with `plant` the
    first 2 * n_out have coord -0.5 and n + 0.5 on one axis each (the other axes inside the grid)."""
    n = np.asarray(grid, dtype=np.float64)
    n_out = len(grid)
    coord = rng.uniform(lo, n + hi, size=(n_points, n_out))
    for d in range(n_out if plant else 0):
        for k, v in enumerate((-0.5, n[d] + 0.5)):
            coord[2 * d + k] = rng.uniform(2, n - 2)
            coord[2 * d + k, d] = v
    y = -1 + 2 * coord / n
    pts = (y - trans) @ rot  # rot has orthonormal rows: rot @ pts + trans = y
    if n_in > n_out:  # any component outside the row space leaves the projection alone
        null = np.linalg.svd(rot)[2][n_out:]
        pts = pts + rng.uniform(-1, 1, size=(n_points, n_in - n_out)) @ null
    return pts


def _reference(c):
    """out grid + (B,) and the six gradients, pose by pose with the single-pose numpy reference in fp64."""
    nb = len(c["rot"])
    pw = c["pw"] if c["pw"] is not None else [None] * nb
    out = np.stack([SR.raster_smooth(c["grid"], c["points"][b], c["rot"][b:b + 1], c["trans"][b:b + 1],
                                     c["bg"][b:b + 1], c["ow"][b:b + 1], pw[b])[..., 0] for b in range(nb)], axis=-1)
    parts = [SR.raster_pullback_smooth(c["g"][..., b:b + 1], c["points"][b], c["rot"][b:b + 1], c["trans"][b:b + 1],
                                       c["ow"][b:b + 1], pw[b]) for b in range(nb)]
    pb = (np.stack([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
          np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]),
          np.concatenate([p[4] for p in parts]), np.stack([p[5] for p in parts]))
    return out, pb


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out):
    """The inputs (fp64 numpy) and the fp64 reference results, computed once and shared; never modified."""
    rng = np.random.default_rng(1000 + 10 * n_in + n_out)
    grid = GRIDS[n_out]
    rot, trans = _poses(rng, B, n_in, n_out)
    pts = np.stack([_cloud(rng, grid, rot[b], trans[b], n_in, P, plant=True) for b in range(B)])
    for b in range(B):  # the cloud does reach the branches it is drawn for
        co = _coords(grid, pts[b], rot[b], trans[b])
        ok = np.all((co >= -1) & (co < np.asarray(grid) + 1), axis=1)
        j0 = np.floor(co[ok]).astype(int)
        assert 0 < ok.sum() < P
        for d in range(n_out):
            assert (j0[:, d] == -1).any() and (j0[:, d] == grid[d]).any()
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, bg=rng.normal(size=B), ow=rng.uniform(0.5, 1.5, size=B),
             pw=rng.uniform(0.5, 1.5, size=(B, P)), g=rng.normal(size=grid + (B,)))
    c["out"], c["pb"] = _reference(c)
    return _freeze(c)


def _dev_args(c, dev, npdt):
    return [T(c[k].astype(npdt), dev) if c[k] is not None else None
            for k in ("points", "rot", "trans", "bg", "ow", "pw")]


def _check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        if a is None and e is None:
            continue
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ 1. forward against the reference
@pytest.mark.parametrize("algo", ["atomic", "tiled", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    out = dpr_amd.raster_smooth_clouds(c["grid"], *_dev_args(c, dev, npdt), algo=algo)
    assert out.shape == c["grid"] + (B,) and out.dtype == tdt
    assert_close(out, c["out"].astype(npdt), tol(npdt, "out"), algo)
    for b in range(B):
        assert_close(out[..., b], c["out"][..., b].astype(npdt), tol(npdt, "out"), f"{algo} plane {b}")
    assert dpr_amd.resolve_algo_smooth_clouds("raster", c["grid"], P, B, n_in) in ("atomic", "tiled")


# ------------------------------------------------------------------ 2. pose-group cuts
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_pose_groups(dev, group, npdt, tdt, n_in, n_out):
    """max_pose_group 1 (pose by pose), 2 (groups of 2 + 2 + 1) and 0 (all five poses in one group)."""
    c = _case(n_in, n_out)
    args = _dev_args(c, dev, npdt)
    need = dpr_amd.workspace_bytes_smooth_clouds("raster", c["grid"], P, B, n_in, tdt, "tiled", max_pose_group=group)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.raster_smooth_clouds(c["grid"], *args, algo="tiled", max_pose_group=group, workspace=ws)
    for b in range(B):
        assert_close(out[..., b], c["out"][..., b].astype(npdt), tol(npdt, "out"), f"group {group} plane {b}")
    # in place, onto a buffer full of NaN
    buf = torch.full_like(out, float("nan"))
    assert dpr_amd.raster_smooth_clouds_(buf, *args, algo="tiled", max_pose_group=group) is buf
    assert_close(buf, c["out"].astype(npdt), tol(npdt, "out"), f"group {group} in place")


# ------------------------------------------------------------------ 3. empty poses
@pytest.mark.parametrize("empty", [0, 2, 4])
@pytest.mark.parametrize("algo,group", [("atomic", 0), ("tiled", 0), ("tiled", 2)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_pose_whose_cloud_lies_outside_the_grid(dev, empty, algo, group, npdt, tdt, n_in, n_out):
    """An empty pose at the start, inside and at the end of a group's start table: its plane is exactly its
    background, the other planes are unaffected."""
    c = _case(n_in, n_out)
    rng = np.random.default_rng(empty)
    pts = c["points"].copy()
    # coord in [n + 2, n + 6) on every axis under the pose's own transform: every point rejected
    pts[empty] = _cloud(rng, c["grid"], c["rot"][empty], c["trans"][empty], n_in, P,
                        lo=np.asarray(c["grid"]) + 2.0, hi=6.0)
    co = _coords(c["grid"], pts[empty], c["rot"][empty], c["trans"][empty])
    assert np.all(np.any(co >= np.asarray(c["grid"]) + 1, axis=1))
    args = _dev_args(c, dev, npdt)
    args[0] = T(pts.astype(npdt), dev)
    out = dpr_amd.raster_smooth_clouds(c["grid"], *args, algo=algo, max_pose_group=group)
    plane = out[..., empty].cpu().numpy()
    assert np.array_equal(plane, np.full(c["grid"], c["bg"][empty].astype(npdt)))
    for b in range(B):
        if b != empty:
            assert_close(out[..., b], c["out"][..., b].astype(npdt), tol(npdt, "out"), f"plane {b}")


# ------------------------------------------------------------------ 4. pullback against the reference
@pytest.mark.parametrize("algo", ["atomic", "auto"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pullback_matches_the_reference(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    assert dpr_amd.resolve_algo_smooth_clouds("pullback", c["grid"], P, B, n_in) == "atomic"
    g = grid_to_dev(c["g"].astype(npdt), dev)
    args = _dev_args(c, dev, npdt)
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
    d_pts, d_rot_cm, d_tr = nan(B, P, n_in), nan(B, n_in, n_out), nan(B, n_out)
    d_bg, d_ow, d_pw = nan(B), nan(B), nan(B, P)
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, *args, algo=algo, ds_dpoints=d_pts,
                                                ds_drotation=d_rot_cm.transpose(1, 2), ds_dtranslation=d_tr,
                                                ds_dbackground=d_bg, ds_dout_weight=d_ow, ds_dpoint_weight=d_pw)
    assert pb.points is d_pts and pb.translation is d_tr and pb.background is d_bg
    assert pb.out_weight is d_ow and pb.point_weight is d_pw and pb.rotation.data_ptr() == d_rot_cm.data_ptr()
    assert pb.rotation.shape == (B, n_out, n_in)
    _check_pullback(pb, c["pb"], npdt, f"{algo} ")
    for b in range(B):  # pose by pose: the norm of one pose's rows does not hide another's
        assert_close(pb.points[b], c["pb"][0][b].astype(npdt), tol(npdt, "points"), f"ds_dpoints[{b}]")
        assert_close(pb.point_weight[b], c["pb"][5][b].astype(npdt), tol(npdt, "points"), f"ds_dpoint_weight[{b}]")
        assert_close(pb.rotation[b], c["pb"][1][b].astype(npdt), tol(npdt, "pose"), f"ds_drotation[{b}]")
    # a rejected point gets exact zeros
    co = _coords(c["grid"], c["points"][1], c["rot"][1], c["trans"][1])
    far = np.nonzero(np.any((co < -1.01) | (co >= np.asarray(c["grid"]) + 1.01), axis=1))[0]
    assert len(far) > 0
    assert bool((pb.points[1][torch.as_tensor(far, device=dev)] == 0).all())
    # the same bits on every run: one thread and one store per value
    again = dpr_amd.raster_pullback_smooth_clouds_(g, *args, algo=algo)
    assert torch.equal(again.points, pb.points) and torch.equal(again.point_weight, pb.point_weight)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_pullback_smooth_clouds_(g, *args, algo="tiled")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_pullback_without_the_point_weight_gradient(dev, npdt, tdt):
    n_in, n_out = 3, 3
    c = _case(n_in, n_out)
    g = grid_to_dev(c["g"].astype(npdt), dev)
    args = _dev_args(c, dev, npdt)
    nb = dpr_amd.raster_pullback_smooth_clouds_(g, *args, point_weight_grad=False)
    assert nb.point_weight is None
    _check_pullback(nb[:5], c["pb"][:5], npdt, "no pw grad ")
    with pytest.raises(ValueError):
        dpr_amd.raster_pullback_smooth_clouds_(g, *args, point_weight_grad=False,
                                               ds_dpoint_weight=torch.empty((B, P), dtype=tdt, device=dev))
    # the flagged C call with ds_dpoint_weight = NULL; every other output starts as NaN
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
    d_pts, d_rot_cm, d_tr, d_bg, d_ow = nan(B, P, n_in), nan(B, n_in, n_out), nan(B, n_out), nan(B), nan(B)
    grid = np.asarray(c["grid"], dtype=np.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pts, rot, trans, _bg, ow, pw = args
    rot_cm = rot.transpose(1, 2).contiguous()
    fn = getattr(_lib.lib(), "dpr_raster_pullback_smooth_clouds_ex_" + ("f32" if npdt == np.float32 else "f64"))
    rc = fn(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _lib.ALGO_ATOMIC,
            _lib.FLAG_NO_POINT_WEIGHT_GRAD, n_in, n_out, grid.ctypes.data_as(ctypes.c_void_p), P, B, p(g), p(pts),
            p(rot_cm), p(trans), p(ow), p(pw), p(d_pts), p(d_rot_cm), p(d_tr), p(d_bg), p(d_ow), None, None, 0)
    torch.cuda.synchronize()
    assert rc == _lib.OK, _lib.last_error()
    _check_pullback((d_pts, d_rot_cm.transpose(1, 2), d_tr, d_bg, d_ow), c["pb"][:5], npdt, "flagged C call ")


# ------------------------------------------------------------------ 5. consistency with the single-pose operator
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_plane_and_rows_of_a_pose_equal_the_single_pose_operator(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    pts, rot, trans, bg, ow, pw = _dev_args(c, dev, npdt)
    g = grid_to_dev(c["g"].astype(npdt), dev)
    outs = {a: dpr_amd.raster_smooth_clouds(c["grid"], pts, rot, trans, bg, ow, pw, algo=a)
            for a in ("atomic", "tiled")}
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, pts, rot, trans, bg, ow, pw)
    for b in range(B):
        single = (pts[b].contiguous(), rot[b:b + 1], trans[b:b + 1], bg[b:b + 1], ow[b:b + 1], pw[b].contiguous())
        for a in ("atomic", "tiled"):
            o1 = dpr_amd.raster_smooth(c["grid"], *single, algo=a)
            assert_close(outs[a][..., b], o1[..., 0].cpu().numpy(), tol(npdt, "out"), f"plane {b}, {a}")
        p1 = dpr_amd.raster_pullback_smooth_(dpr_amd.to_grid_layout(g[..., b:b + 1]), *single)
        assert_close(pb.points[b], p1.points.cpu().numpy(), tol(npdt, "points"), f"ds_dpoints[{b}]")
        assert_close(pb.point_weight[b], p1.point_weight.cpu().numpy(), tol(npdt, "points"), f"ds_dpw[{b}]")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_copies_of_one_cloud_reproduce_the_shared_cloud_operator(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    _pts, rot, trans, bg, ow, _pw = _dev_args(c, dev, npdt)
    one, pw1 = T(c["points"][0].astype(npdt), dev), T(c["pw"][0].astype(npdt), dev)
    rep = one.unsqueeze(0).expand(B, P, n_in).contiguous()
    g = grid_to_dev(c["g"].astype(npdt), dev)
    shared = dpr_amd.raster_smooth(c["grid"], one, rot, trans, bg, ow, pw1, algo="atomic")
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_clouds(c["grid"], rep, rot, trans, bg, ow, pw1, algo=algo)  # shared (P,) weights
        assert_close(out, shared.cpu().numpy(), tol(npdt, "out"), f"B copies, {algo}")
    spb = dpr_amd.raster_pullback_smooth_(g, one, rot, trans, bg, ow, pw1)
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, rep, rot, trans, bg, ow, pw1)
    assert pb.point_weight.shape == (P,)
    assert_close(pb.points.sum(dim=0), spb.points.cpu().numpy(), tol(npdt, "points"), "sum over b of ds_dpoints[b]")
    assert_close(pb.point_weight, spb.point_weight.cpu().numpy(), tol(npdt, "points"), "shared ds_dpoint_weight")
    for name, a, e in (("rotation", pb.rotation, spb.rotation), ("translation", pb.translation, spb.translation),
                       ("background", pb.background, spb.background), ("out_weight", pb.out_weight, spb.out_weight)):
        assert_close(a, e.cpu().numpy(), tol(npdt, "pose"), name)


# ------------------------------------------------------------------ 6. padding
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_cloud_padded_with_zero_weights(dev, npdt, tdt, n_in, n_out):
    """Cloud 1 holds 200 points and 100 rows of padding with point_weight 0 (the padding rows are ordinary points
    of the cloud, inside and outside the grid)."""
    c = _case(n_in, n_out)
    pw = c["pw"].copy()
    pw[1, 200:] = 0
    args = _dev_args(c, dev, npdt)
    args[5] = T(pw.astype(npdt), dev)
    b = 1
    want = SR.raster_smooth(c["grid"], c["points"][b, :200], c["rot"][b:b + 1], c["trans"][b:b + 1],
                            c["bg"][b:b + 1], c["ow"][b:b + 1], pw[b, :200])[..., 0]
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_clouds(c["grid"], *args, algo=algo)
        assert_close(out[..., b], want.astype(npdt), tol(npdt, "out"), f"padded plane, {algo}")
        assert_close(out[..., 0], c["out"][..., 0].astype(npdt), tol(npdt, "out"), f"plane 0, {algo}")
    pb = dpr_amd.raster_pullback_smooth_clouds_(grid_to_dev(c["g"].astype(npdt), dev), *args)
    assert bool((pb.points[b, 200:] == 0).all())
    ref = SR.raster_pullback_smooth(c["g"][..., b:b + 1], c["points"][b, :200], c["rot"][b:b + 1],
                                    c["trans"][b:b + 1], c["ow"][b:b + 1], pw[b, :200])
    assert_close(pb.points[b, :200], ref[0].astype(npdt), tol(npdt, "points"), "ds_dpoints of the 200")
    assert_close(pb.rotation[b], ref[1][0].astype(npdt), tol(npdt, "pose"), "ds_drotation of the padded pose")


# ------------------------------------------------------------------ 7. edge sizes
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_no_poses_and_one_point(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    _pts, rot, trans, bg, ow, _pw = _dev_args(c, dev, npdt)
    grid = c["grid"]
    g = grid_to_dev(c["g"].astype(npdt), dev)
    # P = 0: the background, and empty / zero gradients
    none = torch.zeros((B, 0, n_in), dtype=tdt, device=dev)
    out = dpr_amd.raster_smooth_clouds(grid, none, rot, trans, bg, ow, algo=algo)
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(c["bg"].astype(npdt), grid + (B,)))
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, none, rot, trans, bg, ow)
    assert pb.points.shape == (B, 0, n_in) and pb.point_weight.shape == (B, 0)
    assert bool((pb.rotation == 0).all()) and bool((pb.translation == 0).all()) and bool((pb.out_weight == 0).all())
    assert_close(pb.background, c["g"].reshape(-1, B).sum(axis=0).astype(npdt), tol(npdt, "pose"), "P=0 ds_dbg")
    # B = 0
    e = lambda *s: torch.zeros(s, dtype=tdt, device=dev)
    out = dpr_amd.raster_smooth_clouds(grid, e(0, P, n_in), e(0, n_out, n_in), e(0, n_out), algo=algo)
    assert out.shape == grid + (0,)
    pb = dpr_amd.raster_pullback_smooth_clouds_(dpr_amd.empty_grid(grid, 0, tdt, dev), e(0, P, n_in),
                                                e(0, n_out, n_in), e(0, n_out))
    assert pb.points.shape == (0, P, n_in) and pb.rotation.shape == (0, n_out, n_in)
    # P = 1
    one = dict(c, points=c["points"][:, :1], pw=c["pw"][:, :1])
    want, want_pb = _reference(one)
    out = dpr_amd.raster_smooth_clouds(grid, *_dev_args(one, dev, npdt), algo=algo)
    assert_close(out, want.astype(npdt), tol(npdt, "out"), "P=1")
    _check_pullback(dpr_amd.raster_pullback_smooth_clouds_(g, *_dev_args(one, dev, npdt)), want_pb, npdt, "P=1 ")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_one_pose_with_every_point_in_one_cell(dev, algo, npdt, tdt, n_in, n_out):
    """Pose 1 of three holds 2 000 points in a single cell (on the tiled path one LDS cell serialises them); poses 0
    and 2 are ordinary clouds of 2 000 points."""
    rng = np.random.default_rng(77)
    grid, nb, npts = GRIDS[n_out], 3, 2000
    rot, trans = _poses(rng, nb, n_in, n_out)
    pts = np.stack([_cloud(rng, grid, rot[b], trans[b], n_in, npts) for b in range(nb)])
    cell = np.asarray(grid) // 2 + 0.25
    pts[1] = _cloud(rng, grid, rot[1], trans[1], n_in, npts, lo=cell, hi=cell + 0.5 - np.asarray(grid))
    assert len(np.unique(np.floor(_coords(grid, pts[1], rot[1], trans[1])), axis=0)) == 1
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, bg=rng.normal(size=nb), ow=rng.uniform(0.5, 1.5, size=nb),
             pw=rng.uniform(0.5, 1.5, size=(nb, npts)), g=rng.normal(size=grid + (nb,)))
    want, _ = _reference(c)
    out = dpr_amd.raster_smooth_clouds(grid, *_dev_args(c, dev, npdt), algo=algo)
    for b in range(nb):
        assert_close(out[..., b], want[..., b].astype(npdt), tol(npdt, "out"), f"plane {b}")
    mass = float((out[..., 1].double() - float(c["bg"][1].astype(npdt))).sum())
    assert abs(mass - c["ow"][1] * c["pw"][1].sum()) <= tol(npdt, "out") * abs(c["ow"][1] * c["pw"][1].sum())


# ------------------------------------------------------------------ 8. launch cut
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_more_poses_than_one_launch_axis_holds(dev, npdt, tdt):
    """B = 65 539 poses of 2 points on an (8, 8) grid: the ATOMIC kernels stride the poses over 65 535 rows of
    workgroups, the TILED forward bins all poses as one group (65 539 keys of one tile each).  Every pose is a copy
    of pose 0 except 65 534, 65 535 and 65 538."""
    rng = np.random.default_rng(8)
    n_in, n_out, grid, nb, npts = 2, 2, (8, 8), 65_539, 2
    special = [65_534, 65_535, 65_538]
    rot4, trans4 = _poses(rng, 4, n_in, n_out)
    small = dict(grid=grid, rot=rot4, trans=trans4, bg=rng.normal(size=4), ow=rng.uniform(0.5, 1.5, size=4),
                 points=np.stack([_cloud(rng, grid, rot4[k], trans4[k], n_in, npts, lo=1.0, hi=-1.0) for k in range(4)]),
                 pw=rng.uniform(0.5, 1.5, size=(4, npts)), g=rng.normal(size=grid + (4,)))
    want, want_pb = _reference(small)
    where = np.zeros(nb, dtype=np.int64)  # pose b of the call is row where[b] of `small`
    where[special] = [1, 2, 3]
    big = {k: T(np.ascontiguousarray(small[k][where]).astype(npdt), dev)
           for k in ("points", "rot", "trans", "bg", "ow", "pw")}
    args = [big[k] for k in ("points", "rot", "trans", "bg", "ow", "pw")]
    g = grid_to_dev(np.ascontiguousarray(small["g"][..., where]).astype(npdt), dev)
    rows = [0] + special
    others = torch.as_tensor(np.setdiff1d(np.arange(nb), rows), device=dev)

    def per_pose_error(a, ref0):
        """max over the poses of |a[b] - ref0| / |ref0| (a: (poses, ...), ref0 one pose's values)"""
        d = (a.double() - ref0.double().unsqueeze(0)).flatten(1).norm(dim=1)
        return float(d.max() / ref0.double().norm())

    assert dpr_amd.workspace_bytes_smooth_clouds("raster", grid, npts, nb, n_in, tdt, "tiled") > \
        dpr_amd.workspace_bytes_smooth("raster", grid, npts, 1, n_in, tdt, "tiled")
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_clouds(grid, *args, algo=algo)
        planes = out.movedim(-1, 0)
        for k, b in enumerate(rows):
            assert_close(planes[b], want[..., k].astype(npdt), tol(npdt, "out"), f"{algo} plane {b}")
        assert per_pose_error(planes[others], planes[0]) <= tol(npdt, "out"), algo
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, *args, algo="atomic")
    for name, kind, a, e in zip(FIELDS, KINDS, pb, want_pb):
        for k, b in enumerate(rows):
            assert_close(a[b], e[k].astype(npdt), tol(npdt, kind), f"{name}[{b}]")
        assert per_pose_error(a[others].reshape(len(others), -1), a[0].reshape(-1)) <= tol(npdt, kind), name


# ------------------------------------------------------------------ 9. the exact derivative, fp64
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, n_in, n_out):
    """raster_smooth_clouds_ad in fp64 on an 8^N grid, 2 poses of 10 points: central differences with h = 1e-6 of
    sum(out * g) in all six arguments, within 1e-6 * max|gradient| (the bound of tests/test_smooth_gpu.py)."""
    rng = np.random.default_rng(11)
    nb, npts, grid = 2, 10, (8,) * n_out
    rot, trans = _poses(rng, nb, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(nb, npts, n_in)), rot, trans, rng.normal(size=nb),
            rng.uniform(0.5, 1.5, size=nb), rng.uniform(0.5, 1.5, size=(nb, npts))]
    g = grid_to_dev(rng.normal(size=grid + (nb,)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    out = dpr_amd.raster_smooth_clouds_ad(grid, *xs)
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
                up = float((dpr_amd.raster_smooth_clouds(grid, *xs) * g).sum())
                flat[i] = keep - h
                dn = float((dpr_amd.raster_smooth_clouds(grid, *xs) * g).sum())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (FIELDS[k], err, scale)
        # a weight shared by all poses receives the sum over the poses of its per-pose gradients
        shared = vals[5][0]
        per_pose = dpr_amd.raster_pullback_smooth_clouds_(
            g, xs[0], xs[1], xs[2], xs[3], xs[4], T(np.broadcast_to(shared, (nb, npts)).copy(), dev)).point_weight
    pw = torch.tensor(shared, dtype=torch.float64, device=dev, requires_grad=True)
    (dpr_amd.raster_smooth_clouds_ad(grid, xs[0].detach(), xs[1].detach(), xs[2].detach(), xs[3].detach(),
                                     xs[4].detach(), pw, algo="tiled") * g).sum().backward()
    assert pw.grad.shape == (npts,)
    assert_close(pw.grad, per_pose.sum(dim=0).cpu().numpy(), 1e-12, "shared point_weight")


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_gradient_is_continuous_across_a_cell_face(dev, n_in, n_out):
    """Every point of cloud 1 sits 1e-9 cells either side of a cell face of axis 0 (fp64): the gradients of the two
    calls differ by less than 1e-6 * max|gradient|."""
    rng = np.random.default_rng(5)
    grid, nb, npts = (8,) * n_out, 3, 6
    g = grid_to_dev(rng.normal(size=grid + (nb,)), dev)
    rot, trans = _poses(rng, nb, n_in, n_out)
    pts = np.stack([_cloud(rng, grid, rot[b], trans[b], n_in, npts, lo=1.0, hi=-1.0) for b in range(nb)])
    face = np.array([2, 3, 4, 5, 6, 3], dtype=np.float64)
    base = rng.uniform(1, 7, size=(npts, n_out))
    sides = []
    for eps in (-1e-9, 1e-9):
        coord = base.copy()
        coord[:, 0] = face + eps
        y = -1 + 2 * coord / 8
        p = pts.copy()
        p[1] = (y - trans[1]) @ rot[1]
        sides.append(p)
    lo, hi = sides
    assert np.all(np.floor(_coords(grid, lo[1], rot[1], trans[1])[:, 0]) + 1
                  == np.floor(_coords(grid, hi[1], rot[1], trans[1])[:, 0]))
    run = lambda p: dpr_amd.raster_pullback_smooth_clouds_(g, T(p, dev), T(rot, dev), T(trans, dev))
    pa, pb = run(lo), run(hi)
    scale = max(float(a.abs().max()) for a in pa)
    for a, b in zip(pa, pb):
        assert float((a - b).abs().max()) < 1e-6 * scale
