"""Smooth sampling at per-pose clouds on the GPU (dpr_amd.sample_smooth_clouds / sample_smooth_clouds_pullback_ /
sample_smooth_clouds_ad; include/dpr.h, SMOOTH SAMPLING, PER-POSE CLOUDS; kernels: csrc/dpr_sample_smooth_clouds.hip)
against tests/sample_smooth_clouds_reference.py, the numpy smooth sampling reference composed per pose and evaluated
in fp64.  Tolerances: tol(npdt, kind) of tests/test_parity_gpu.py (fp64 1e-10; fp32 5e-5 `out` for images, 1e-4
`points` for values and point gradients, 1e-3 `pose` for pose gradients), norm-wise: per plane for images, per pose
for pose gradients.

Shapes: the smallest that reach the hazards.  Grids (70, 19) and (18, 9, 10): 2 x 2 and 2 x 2 x 2 tiles of the tiled
path (64 x 16, 16 x 8 x 8), no axis a multiple of its tile; (5, 7): smaller than a tile.  P = 777 (four blocks of 256,
the last partial, and a partial wave), B = 3.  The clouds are deformed copies of one cloud that is drawn in the frame
of pose 0 with coordinates spanning -2 .. n + 2 on every axis and points planted at j0 = -1 and j0 = n of every axis:
a point is accepted under pose 0 and its copy rejected under another pose, and some points lie outside the grid."""
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from tests import sample_smooth_clouds_reference as SCR
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol
from tests.test_smooth_clouds_gpu import _cloud, _coords, _poses

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (70, 19), 3: (18, 9, 10)}
SMALL = (5, 7)
FIELDS = ("image", "points", "rotation", "translation")
KINDS = ("out", "points", "pose", "pose")
P, B = 777, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _grids(n_out):
    return [GRIDS[n_out]] + ([SMALL] if n_out == 2 else [])


def _accepted(c):
    """(B, P) bool: point p of cloud b is accepted under pose b."""
    n = np.asarray(c["grid"])
    co = np.stack([_coords(c["grid"], c["points"][b], c["rot"][b], c["trans"][b]) for b in range(len(c["rot"]))])
    return np.all((co >= -1) & (co < n + 1), axis=2)


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out, grid=None, nb=B, n_points=P, seed=0):
    """The inputs (fp64 numpy) and the fp64 reference results, computed once and shared; never modified."""
    rng = np.random.default_rng(5000 + 10 * n_in + n_out + 100 * nb + 1000 * seed)
    grid = GRIDS[n_out] if grid is None else tuple(grid)
    rot, trans = _poses(rng, nb, n_in, n_out)
    base = _cloud(rng, grid, rot[0], trans[0], n_in, n_points, plant=True)
    pts = base[None] + rng.normal(scale=0.02, size=(nb, n_points, n_in))
    pts[0] = base
    c = dict(grid=grid, points=pts, rot=rot, trans=trans, image=rng.normal(size=grid + (nb,)),
             dv=rng.normal(size=(nb, n_points)))
    c["values"] = SCR.sample_smooth_clouds(c["image"], pts, rot, trans)
    c["pb"] = SCR.sample_smooth_clouds_pullback(c["dv"], c["image"], pts, rot, trans)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dev_args(c, dev, npdt):
    return [grid_to_dev(c["image"].astype(npdt), dev)] + [T(c[k].astype(npdt), dev) for k in ("points", "rot", "trans")]


def _check_pullback(pb, ref, npdt, what=""):
    """Norm-wise: images per plane, pose gradients per pose, point gradients per cloud and as a whole."""
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        if a is None:
            continue
        assert tuple(a.shape) == e.shape, f"{what}{name}: shape {tuple(a.shape)} != {e.shape}"
        for b in range(e.shape[-1] if name == "image" else e.shape[0]):
            if name == "image":
                assert_close(a[..., b], e[..., b].astype(npdt), tol(npdt, kind), f"{what}ds_dimage[..., {b}]")
            else:
                assert_close(a[b], e[b].astype(npdt), tol(npdt, kind), f"{what}ds_d{name}[{b}]")
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}ds_d{name}")


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_and_pullback_match_the_reference(dev, npdt, tdt, n_in, n_out):
    for grid in _grids(n_out):
        c = _case(n_in, n_out, grid=grid)
        n = np.asarray(grid)
        # the clouds do reach the branches they are drawn for
        acc = _accepted(c)
        assert acc.shape == (B, P) and P == 777
        assert (acc.any(axis=0) & ~acc.all(axis=0)).sum() > 10  # rejected under one pose, accepted under another
        assert all(0 < acc[b].sum() < P for b in range(B))       # every pose rejects some points ...
        assert np.all(c["values"][~acc] == 0) and np.all(c["pb"][1][~acc] == 0)
        j0 = np.floor(_coords(grid, c["points"][0][acc[0]], c["rot"][0], c["trans"][0])).astype(int)
        for d in range(n_out):                                   # ... and accepts points outside the grid
            assert (j0[:, d] == -1).any() and (j0[:, d] == n[d]).any()
        args = _dev_args(c, dev, npdt)
        rej = torch.as_tensor(~acc, device=dev)
        for algo in ("atomic", "auto"):
            v = dpr_amd.sample_smooth_clouds(*args, algo=algo)
            assert v.shape == (B, P) and v.dtype == tdt and v.is_contiguous()
            assert_close(v, c["values"].astype(npdt), tol(npdt, "points"), f"{grid} {algo} values")
            for b in range(B):
                assert_close(v[b], c["values"][b].astype(npdt), tol(npdt, "points"), f"{grid} {algo} values[{b}]")
            assert bool((v[rej] == 0).all())
        dv = T(c["dv"].astype(npdt), dev)
        for algo in ("atomic", "tiled", "auto"):
            pb = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, algo=algo)
            assert pb.image.shape == grid + (B,) and pb.image.dtype == tdt
            assert pb.image.permute(*reversed(range(pb.image.ndim))).is_contiguous()
            assert pb.points.shape == (B, P, n_in) and pb.points.is_contiguous()
            assert pb.rotation.shape == (B, n_out, n_in) and pb.translation.shape == (B, n_out)
            _check_pullback(pb, c["pb"], npdt, f"{grid} {algo} ")
            assert bool((pb.points[rej] == 0).all())
        assert dpr_amd.resolve_algo_sample_smooth_clouds("pullback", grid, P, B, n_in) == "atomic"


# ------------------------------------------------------------------ 2. bit-for-bit rows
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_rows_have_the_bits_of_the_single_pose_calls(dev, npdt, tdt, n_in, n_out):
    """values[b] == sample_smooth(image[..., b], points[b], R_b, t_b) and ds_dpoints[b] == the single-pose
    sample_smooth_pullback_(need=("points",), algo="atomic"): no sum across threads, one order of operations."""
    for grid in _grids(n_out):
        c = _case(n_in, n_out, grid=grid)
        img, pts, rot, trans = _dev_args(c, dev, npdt)
        dv = T(c["dv"].astype(npdt), dev)
        v = dpr_amd.sample_smooth_clouds(img, pts, rot, trans)
        d_pts = {a: dpr_amd.sample_smooth_clouds_pullback_(dv, img, pts, rot, trans, need=("points",), algo=a).points
                 for a in ("atomic", "tiled")}
        full = dpr_amd.sample_smooth_clouds_pullback_(dv, img, pts, rot, trans, algo="atomic").points
        for b in range(B):
            plane = dpr_amd.to_grid_layout(img[..., b])
            assert torch.equal(v[b], dpr_amd.sample_smooth(plane, pts[b], rot[b], trans[b])), f"{grid}: row {b}"
            one = dpr_amd.sample_smooth_pullback_(dv[b], plane, pts[b], rot[b], trans[b], need=("points",),
                                                  algo="atomic").points
            assert one.shape == (P, n_in)
            for a, g in d_pts.items():
                assert torch.equal(g[b], one), f"{grid} {a}: ds_dpoints[{b}]"
            assert torch.equal(full[b], one), f"{grid}: ds_dpoints[{b}] of a call with every output"


# ------------------------------------------------------------------ 3. the same cloud for every pose
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_the_same_cloud_for_every_pose_is_batched_sample_smooth(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    img, pts, rot, trans = _dev_args(c, dev, npdt)
    one = pts[0].contiguous()
    same = one[None].expand(B, P, n_in).contiguous()
    dv = T(c["dv"].astype(npdt), dev)
    v = dpr_amd.sample_smooth_clouds(img, same, rot, trans)
    want = dpr_amd.sample_smooth(img, one, rot, trans)  # (P, B)
    assert_close(v, want.t().cpu().numpy(), tol(npdt, "points"), "values")
    for algo in ("atomic", "tiled"):
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv, img, same, rot, trans, algo=algo)
        ref = dpr_amd.sample_smooth_pullback_(dv.t(), img, one, rot, trans, algo=algo)
        for b in range(B):
            assert_close(pb.image[..., b], ref.image[..., b].cpu().numpy(), tol(npdt, "out"), f"{algo} image {b}")
            assert_close(pb.rotation[b], ref.rotation[b].cpu().numpy(), tol(npdt, "pose"), f"{algo} rotation {b}")
            assert_close(pb.translation[b], ref.translation[b].cpu().numpy(), tol(npdt, "pose"), f"{algo} trans {b}")
        assert_close(pb.points.sum(dim=0), ref.points.cpu().numpy(), tol(npdt, "points"), f"{algo} points")


# ------------------------------------------------------------------ 4. ds_dimage is the smooth cloud splat
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_image_gradient_is_the_smooth_cloud_splat_of_ds_dvalues(dev, algo, npdt, tdt, n_in, n_out):
    for grid in _grids(n_out):
        c = _case(n_in, n_out, grid=grid)
        img, pts, rot, trans = _dev_args(c, dev, npdt)
        dv = T(c["dv"].astype(npdt), dev)
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv, img, pts, rot, trans, need=("image",), algo=algo)
        assert pb.points is None and pb.rotation is None and pb.translation is None
        want = dpr_amd.raster_smooth_clouds(grid, pts, rot, trans, None, None, dv, algo=algo)
        for b in range(B):
            assert_close(pb.image[..., b], want[..., b].cpu().numpy(), tol(npdt, "out"), f"{grid} {algo}: plane {b}")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_adjoint_identity_on_the_device(dev, npdt, tdt, n_in, n_out):
    """sum_v out[v, b] * image[v, b] == sum_p pw[b, p] * values[b, p] per pose, for out = raster_smooth_clouds(pw)
    without background; relative to the sum of the magnitudes of the terms, within tol(npdt, "out").  The sums
    themselves are taken in fp64."""
    c = _case(n_in, n_out)
    img, pts, rot, trans = _dev_args(c, dev, npdt)
    pw = T(c["dv"].astype(npdt), dev)
    values = dpr_amd.sample_smooth_clouds(img, pts, rot, trans)
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth_clouds(c["grid"], pts, rot, trans, None, None, pw, algo=algo)
        for b in range(B):
            lt, rt = out[..., b].double() * img[..., b].double(), pw[b].double() * values[b].double()
            lhs, rhs = float(lt.sum()), float(rt.sum())
            mag = float(lt.abs().sum()) + float(rt.abs().sum())
            assert mag > 0 and abs(lhs - rhs) <= tol(npdt, "out") * mag, (algo, b, lhs, rhs, mag)


# ------------------------------------------------------------------ 5. pose groups
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_pose_groups_agree(dev, npdt, tdt, n_in, n_out):
    """B = 5 with max_pose_group 1, 2 and the default: groups of 1 x 5, 2 + 2 + 1 and 5.  All agree with the reference
    and with each other; the workspace a call needs is the splat's for the same group."""
    c = _case(n_in, n_out, nb=5)
    args = _dev_args(c, dev, npdt)
    dv = T(c["dv"].astype(npdt), dev)
    got, needs = {}, {}
    for group in (1, 2, 0):
        needs[group] = dpr_amd._pkg.workspace_bytes_sample_smooth_clouds("pullback", c["grid"], P, 5, n_in, tdt, "tiled",
                                                                    max_pose_group=group)
        assert needs[group] == dpr_amd.workspace_bytes_smooth_clouds("raster", c["grid"], P, 5, n_in, tdt, "tiled",
                                                                     max_pose_group=group)
        ws = torch.empty(needs[group], dtype=torch.uint8, device=dev)
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, algo="tiled", max_pose_group=group, workspace=ws)
        _check_pullback(pb, c["pb"], npdt, f"group {group}: ")
        got[group] = pb
    assert needs[1] < needs[2] < needs[0]
    for group in (1, 2):
        for b in range(5):
            assert_close(got[group].image[..., b], got[0].image[..., b].cpu().numpy(), tol(npdt, "out"),
                         f"group {group} against the default: plane {b}")
        for name in ("points", "rotation", "translation"):  # (the point kernel does not see the groups)
            kind = "points" if name == "points" else "pose"
            assert_close(getattr(got[group], name), getattr(got[0], name).cpu().numpy(), tol(npdt, kind), name)
    # the flag is ignored off the tiled pullback
    v = dpr_amd.sample_smooth_clouds(*args)
    assert torch.equal(dpr_amd.sample_smooth_clouds(*args, max_pose_group=2), v)
    pa = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, algo="atomic", max_pose_group=2)
    _check_pullback(pa, c["pb"], npdt, "atomic, max_pose_group=2: ")


# ------------------------------------------------------------------ 6. need subsets
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_need_subsets_write_only_their_buffers(dev, algo, npdt, tdt):
    """The four outputs lie back to back in one arena filled with 7.5: a call writes the ones in `need`, returns them
    by identity, and leaves every other byte of the arena alone."""
    n_in, n_out = 3, 3
    c = _case(n_in, n_out)
    grid = c["grid"]
    args = _dev_args(c, dev, npdt)
    dv = T(c["dv"].astype(npdt), dev)
    G = int(np.prod(grid))
    sizes = dict(image=B * G, points=B * P * n_in, rotation=B * n_in * n_out, translation=B * n_out)
    for need in (("image",), ("points",), ("rotation",), ("translation",), ("rotation", "translation"),
                 ("image", "points"), FIELDS):
        arena = torch.full((sum(sizes.values()),), 7.5, dtype=tdt, device=dev)
        parts, o = {}, 0
        for name in FIELDS:
            parts[name] = arena[o:o + sizes[name]]
            o += sizes[name]
        bufs = dict(image=parts["image"].view((B,) + grid[::-1]).permute(3, 2, 1, 0),
                    points=parts["points"].view(B, P, n_in),
                    rotation=parts["rotation"].view(B, n_in, n_out).transpose(1, 2),
                    translation=parts["translation"].view(B, n_out))
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv, *args, need=need, algo=algo,
                                                    **{f"ds_d{name}": bufs[name] for name in need})
        for name, e in zip(FIELDS, c["pb"]):
            got = getattr(pb, name)
            if name in need:
                assert got.data_ptr() == bufs[name].data_ptr()
            else:
                assert got is None
                assert bool((parts[name] == 7.5).all()), f"{need}: {name} was written"
        _check_pullback(pb, c["pb"], npdt, f"{algo} {need}: ")


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
def test_image_gradient_without_the_image(dev, algo):
    c = _case(3, 2)
    npdt = np.float32
    _img, pts, rot, trans = _dev_args(c, dev, npdt)
    dv = T(c["dv"].astype(npdt), dev)
    pull = dpr_amd.sample_smooth_clouds_pullback_
    pb = pull(dv, None, pts, rot, trans, need=("image",), algo=algo, grid_size=c["grid"])
    _check_pullback(pb, c["pb"], npdt, "image=None, grid_size: ")
    buf = dpr_amd.empty_grid(c["grid"], B, torch.float32, dev)
    pb = pull(dv, None, pts, rot, trans, need=("image",), algo=algo, ds_dimage=buf)
    assert pb.image is buf and pb.points is None
    _check_pullback(pb, c["pb"], npdt, "image=None, ds_dimage: ")
    with pytest.raises(ValueError):
        pull(dv, None, pts, rot, trans, algo=algo, grid_size=c["grid"])
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv, None, pts, rot, trans, need=("image",), algo=algo,
             ds_dimage=dpr_amd.empty_grid(c["grid"], B + 1, torch.float32, dev))
    with pytest.raises(dpr_amd.DimensionMismatch):
        pull(dv[:, :-1], _img, pts, rot, trans, algo=algo)
    # a refused call leaves its outputs alone
    sentinel = torch.full((B, P), 7.5, device=dev)
    for bad in ("tiled", "chunked", "ordered"):
        with pytest.raises(dpr_amd.DprError) as e:
            dpr_amd.sample_smooth_clouds_(sentinel, _img, pts, rot, trans, algo=bad)
        assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_clouds_(torch.full((P, B), 7.5, device=dev).t(), _img, pts, rot, trans)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.5).all())


# ------------------------------------------------------------------ 7. edges
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_no_poses_one_point_a_nan_point_and_a_cloud_outside(dev, algo, npdt, tdt, n_in, n_out):
    rng = np.random.default_rng(13)
    grid = (8,) * n_out
    rot, trans = _poses(rng, B, n_in, n_out)
    image = rng.normal(size=grid + (B,))
    img, R, t = grid_to_dev(image.astype(npdt), dev), T(rot.astype(npdt), dev), T(trans.astype(npdt), dev)
    pull = dpr_amd.sample_smooth_clouds_pullback_
    z = lambda *sh: torch.zeros(sh, dtype=tdt, device=dev)
    # P = 0: empty values and point gradients; the other gradients are zero
    assert dpr_amd.sample_smooth_clouds(img, z(B, 0, n_in), R, t).shape == (B, 0)
    pb = pull(z(B, 0), img, z(B, 0, n_in), R, t, algo=algo)
    assert pb.points.shape == (B, 0, n_in) and pb.image.shape == grid + (B,)
    for g in (pb.image, pb.rotation, pb.translation):
        assert bool((g == 0).all())
    # B = 0: everything is empty, and nothing is written
    img0 = dpr_amd.empty_grid(grid, 0, tdt, dev)
    assert dpr_amd.sample_smooth_clouds(img0, z(0, 5, n_in), z(0, n_out, n_in), z(0, n_out)).shape == (0, 5)
    pb = pull(z(0, 5), img0, z(0, 5, n_in), z(0, n_out, n_in), z(0, n_out), algo=algo)
    assert pb.points.shape == (0, 5, n_in) and pb.rotation.shape == (0, n_out, n_in)
    assert pb.image.shape == grid + (0,) and pb.translation.shape == (0, n_out)
    # one point per cloud
    one = rng.uniform(-0.5, 0.5, size=(B, 1, n_in))
    dv1 = rng.normal(size=(B, 1))
    v = dpr_amd.sample_smooth_clouds(img, T(one.astype(npdt), dev), R, t)
    assert_close(v, SCR.sample_smooth_clouds(image, one, rot, trans).astype(npdt), tol(npdt, "points"), "one point")
    pb = pull(T(dv1.astype(npdt), dev), img, T(one.astype(npdt), dev), R, t, algo=algo)
    _check_pullback(pb, SCR.sample_smooth_clouds_pullback(dv1, image, one, rot, trans), npdt, "one point: ")
    # a NaN point in cloud 1: value 0, zero gradients, and the pose sums of its block are those without it
    n_pts = 5
    pts = rng.uniform(-0.9, 0.9, size=(B, n_pts, n_in))
    dv = rng.normal(size=(B, n_pts))
    ref_pts, ref_dv = pts.copy(), dv.copy()
    ref_dv[1, 2] = 0  # (the reference of "not there": the point as it was, with nothing to pull back)
    pts[1, 2, 0] = np.nan
    v = dpr_amd.sample_smooth_clouds(img, T(pts.astype(npdt), dev), R, t)
    assert float(v[1, 2]) == 0 and bool(torch.isfinite(v).all())
    want = SCR.sample_smooth_clouds(image, ref_pts, rot, trans)
    want[1, 2] = 0
    assert_close(v, want.astype(npdt), tol(npdt, "points"), "NaN point: values")
    pb = pull(T(dv.astype(npdt), dev), img, T(pts.astype(npdt), dev), R, t, algo=algo)
    assert bool((pb.points[1, 2] == 0).all()) and all(bool(torch.isfinite(g).all()) for g in pb)
    _check_pullback(pb, SCR.sample_smooth_clouds_pullback(ref_dv, image, ref_pts, rot, trans), npdt, "NaN point: ")
    # cloud 1 entirely outside the grid (coord 10.4 on every axis of its own pose): an exact-zero row, plane and pose
    # gradients; the other poses as ever
    far = ref_pts.copy()
    far[1] = (np.full((n_pts, n_out), 1.6) - trans[1]) @ rot[1]
    assert not _accepted(dict(grid=grid, points=far, rot=rot, trans=trans))[1].any()
    v = dpr_amd.sample_smooth_clouds(img, T(far.astype(npdt), dev), R, t)
    assert bool((v[1] == 0).all()) and bool((v[0] != 0).any())
    pb = pull(T(dv.astype(npdt), dev), img, T(far.astype(npdt), dev), R, t, algo=algo)
    assert bool((pb.rotation[1] == 0).all()) and bool((pb.translation[1] == 0).all())
    assert bool((pb.points[1] == 0).all()) and bool((pb.image[..., 1] == 0).all())
    _check_pullback(pb, SCR.sample_smooth_clouds_pullback(dv, image, far, rot, trans), npdt, "a cloud outside: ")


def test_more_poses_than_rows_of_blocks(dev):
    """B = 65 537 poses of one point each on a (4, 4) grid: the poses are strided over 65 535 rows of blocks, so rows
    0 and 1 of the launch take a second pose.  A few poses against the reference; all of them against the same op on
    two halves of the batch, neither of which reaches the cap.  With one point and one block per pose every output is
    the work of one thread: equal bit for bit."""
    nb, n_in, n_out, grid = 65537, 2, 2, (4, 4)
    rng = np.random.default_rng(31)
    ang = rng.uniform(0, 2 * np.pi, size=nb)
    rot = np.stack([np.stack([np.cos(ang), -np.sin(ang)], -1), np.stack([np.sin(ang), np.cos(ang)], -1)], -2)
    trans = rng.uniform(-0.1, 0.1, size=(nb, n_out))
    pts = rng.uniform(-0.7, 0.7, size=(nb, 1, n_in))
    image, dv = rng.normal(size=grid + (nb,)), rng.normal(size=(nb, 1))
    f = np.float32
    img, p, R, t, d = grid_to_dev(image.astype(f), dev), T(pts.astype(f), dev), T(rot.astype(f), dev), \
        T(trans.astype(f), dev), T(dv.astype(f), dev)
    v = dpr_amd.sample_smooth_clouds(img, p, R, t)
    pb = dpr_amd.sample_smooth_clouds_pullback_(d, img, p, R, t, algo="atomic")
    assert v.shape == (nb, 1) and bool((v != 0).all())
    pick = np.array([0, 1, 2, 40000, 65534, 65535, 65536])
    want = SCR.sample_smooth_clouds(image[..., pick], pts[pick], rot[pick], trans[pick])
    assert_close(v[pick], want.astype(f), tol(f, "points"), "values of the picked poses")
    ref = SCR.sample_smooth_clouds_pullback(dv[pick], image[..., pick], pts[pick], rot[pick], trans[pick])
    sel = torch.as_tensor(pick, device=dev)
    _check_pullback((pb.image[..., sel], pb.points[sel], pb.rotation[sel], pb.translation[sel]), ref, f, "picked: ")
    cut = 40000
    for lo, hi in ((0, cut), (cut, nb)):
        half = [dpr_amd.to_grid_layout(img[..., lo:hi]), p[lo:hi], R[lo:hi], t[lo:hi]]
        assert torch.equal(v[lo:hi], dpr_amd.sample_smooth_clouds(*half))
        hb = dpr_amd.sample_smooth_clouds_pullback_(d[lo:hi], *half, algo="atomic")
        assert torch.equal(pb.image[..., lo:hi], hb.image) and torch.equal(pb.points[lo:hi], hb.points)
        assert torch.equal(pb.rotation[lo:hi], hb.rotation) and torch.equal(pb.translation[lo:hi], hb.translation)


# ------------------------------------------------------------------ 8. derivative tests on the device
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, algo, n_in, n_out):
    """sample_smooth_clouds_ad in fp64 on an 8^N grid with 3 clouds of 6 points: central differences with h = 1e-6 of
    sum(values * dv) in image, points, rotation and translation, within 1e-6 * max|gradient| (the bound of
    tests/test_sample_smooth_gpu.py)."""
    rng = np.random.default_rng(11)
    nb, n_pts, grid = 3, 6, (8,) * n_out
    rot, trans = _poses(rng, nb, n_in, n_out)
    vals = [rng.normal(size=grid + (nb,)), rng.uniform(-1.1, 1.1, size=(nb, n_pts, n_in)), rot, trans]
    dv = T(rng.normal(size=(nb, n_pts)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    (dpr_amd.sample_smooth_clouds_ad(*xs, algo=algo) * dv).sum().backward()
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
                up = float((dpr_amd.sample_smooth_clouds(*xs) * dv).sum())
                flat[i] = keep - h
                dn = float((dpr_amd.sample_smooth_clouds(*xs) * dv).sum())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (FIELDS[k], err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_values_and_gradients_are_continuous_across_a_cell_face(dev, n_in, n_out):
    """Cloud 1 of 2: six points 1e-9 of a cell either side of an integer coord (fp64).  Values and all four gradients
    differ by less than 1e-6 * max|gradient| and agree with the reference on both sides; cloud 0, which does not move,
    keeps its bits."""
    rng = np.random.default_rng(5)
    grid = (8,) * n_out
    image = rng.normal(size=grid + (2,))
    rot, trans = np.stack([np.eye(n_out, n_in)] * 2), np.zeros((2, n_out))
    base = rng.uniform(-0.5, 0.5, size=(2, 6, n_in))
    base[1, :, 0] = -1 + 2.0 * np.array([2, 3, 4, 5, 6, 3]) / grid[0]
    lo, hi = base.copy(), base.copy()
    lo[1, :, 0] -= 1e-9 * 2 / grid[0]
    hi[1, :, 0] += 1e-9 * 2 / grid[0]
    assert np.all(np.floor((lo[1, :, 0] + 1) * 4) + 1 == np.floor((hi[1, :, 0] + 1) * 4))
    dv = rng.normal(size=(2, 6))
    img_d, dv_d, R, t = grid_to_dev(image, dev), T(dv, dev), T(rot, dev), T(trans, dev)
    res = []
    for pts in (lo, hi):
        v = dpr_amd.sample_smooth_clouds(img_d, T(pts, dev), R, t)
        pb = dpr_amd.sample_smooth_clouds_pullback_(dv_d, img_d, T(pts, dev), R, t)
        assert_close(v, SCR.sample_smooth_clouds(image, pts, rot, trans), 1e-10, "values")
        _check_pullback(pb, SCR.sample_smooth_clouds_pullback(dv, image, pts, rot, trans), np.float64)
        res.append((v,) + tuple(pb))
    scale = max(float(a.abs().max()) for a in res[0][1:])
    for name, a, b in zip(("values",) + FIELDS, *res):
        assert float((a - b).abs().max()) < 1e-6 * scale, name
    assert torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][2][0], res[1][2][0])
