"""The smooth splat of rigid bodies on the GPU (dpr_amd.raster_smooth_bodies / raster_pullback_smooth_bodies_ /
raster_smooth_bodies_ad; include/dpr.h, SMOOTH SPLAT, RIGID BODIES; kernels: csrc/dpr_smooth_bodies.hip) against
tests/smooth_bodies_reference.py, the numpy smooth reference composed per body and evaluated in fp64.  Tolerances:
tol(npdt, kind) of tests/test_parity_gpu.py (fp64 1e-10; fp32 5e-5 `out`, 1e-4 point gradients, 1e-3 pose gradients),
norm-wise, the pose gradients per (image, body).

Shapes: the smallest that reach the hazards.  Grids (70, 19) and (18, 9, 10): 2 x 2 and 2 x 2 x 2 tiles of the tiled
forward (64 x 16, 16 x 8 x 8), no axis a multiple of its tile; (5, 7): smaller than a tile.  P = 777 (four blocks of
256, the last partial), B = 3, K = 3.  Body k is drawn in the frame of pose (0, k) so that its coordinates span
-2 .. n + 2 on every axis, with points planted at j0 = -1 and j0 = n of every axis (accepted, their tile is that of
the clamped cell); the other images see the cloud under unrelated poses, so that points are rejected in one image and
accepted in another."""
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_bodies_reference as ref
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol
from tests.test_smooth_clouds_gpu import _cloud, _coords, _poses

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (70, 19), 3: (18, 9, 10)}
SMALL = (5, 7)
FWD = ("atomic", "tiled")
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")
MIX = (256, 64, 64, 100, 156)  # body sizes of the wave / block mixes: P = 640


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _accepted(c):
    """(B, P) bool: point p is accepted in image b (its body inside [0, K) and its coord inside [-1, n + 1))."""
    B, K = c["rot"].shape[:2]
    n = np.asarray(c["grid"])
    acc = np.zeros((B, len(c["body"])), dtype=bool)
    for b in range(B):
        for k in range(K):
            idx = np.flatnonzero(c["body"] == k)
            co = _coords(c["grid"], c["points"][idx], c["rot"][b, k], c["trans"][b, k])
            acc[b, idx] = np.all((co >= -1) & (co < n + 1), axis=1)
    return acc


def _with_reference(c):
    c["out"] = ref.raster(c["grid"], c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    c["pb"] = ref.raster_pullback(c["g"], c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(n_in, n_out, grid=None, sizes=(259, 259, 259), B=3, order="sorted", seed=0):
    """The inputs (fp64 numpy) and the fp64 reference results, computed once and shared; never modified.  `sizes`:
    points per body, in body order; order "shuffled": the same cloud under a random permutation."""
    rng = np.random.default_rng(2000 + 100 * seed + 10 * n_in + n_out)
    grid = GRIDS[n_out] if grid is None else tuple(grid)
    K, P = len(sizes), int(sum(sizes))
    rot, trans = _poses(rng, B * K, n_in, n_out)
    rot, trans = rot.reshape(B, K, n_out, n_in), trans.reshape(B, K, n_out)
    pts = np.concatenate([_cloud(rng, grid, rot[0, k], trans[0, k], n_in, sizes[k], plant=sizes[k] >= 2 * n_out)
                          for k in range(K)])
    body = np.repeat(np.arange(K), sizes)
    pw = rng.uniform(0.5, 1.5, size=P)
    if order == "shuffled":
        perm = np.random.default_rng(7).permutation(P)
        pts, body, pw = pts[perm], body[perm], pw[perm]
    c = dict(grid=grid, points=pts, body=body, rot=rot, trans=trans, bg=rng.normal(size=B),
             ow=rng.uniform(0.5, 1.5, size=B), pw=pw, g=rng.normal(size=grid + (B,)), B=B, K=K, P=P)
    return _with_reference(c)


def _args(c, dev, npdt, body_dtype=torch.int64):
    f = lambda k: T(c[k].astype(npdt), dev) if c[k] is not None else None
    return [f("points"), torch.as_tensor(np.array(c["body"]), device=dev).to(body_dtype), f("rot"), f("trans"),
            f("bg"), f("ow"), f("pw")]


def _check_pullback(pb, want, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, want):
        if a is None:
            continue
        if name in ("rotation", "translation"):  # per (image, body): the norm of one body does not hide another's
            assert tuple(a.shape) == e.shape, name
            for b in range(e.shape[0]):
                for k in range(e.shape[1]):
                    assert_close(a[b, k], e[b, k].astype(npdt), tol(npdt, kind), f"{what}ds_d{name}[{b}, {k}]")
        else:
            assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}ds_d{name}")


def _grids(n_out):
    return [GRIDS[n_out]] + ([SMALL] if n_out == 2 else [])


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_and_pullback_match_the_reference(dev, order, npdt, tdt, n_in, n_out):
    for grid in _grids(n_out):
        c = _case(n_in, n_out, grid=grid, order=order)
        assert c["P"] == 777 and c["B"] == 3 and c["K"] == 3
        # the cloud does reach the branches it is drawn for
        acc = _accepted(c)
        assert (acc.any(axis=0) & ~acc.all(axis=0)).any()  # rejected in one image, accepted in another
        for k in range(3):
            idx = np.flatnonzero((c["body"] == k) & acc[0])
            j0 = np.floor(_coords(grid, c["points"][idx], c["rot"][0, k], c["trans"][0, k])).astype(int)
            for d in range(n_out):
                assert (j0[:, d] == -1).any() and (j0[:, d] == grid[d]).any()
        assert (np.diff(c["body"]) >= 0).all() == (order == "sorted")
        args = _args(c, dev, npdt)
        for algo in FWD + ("auto",):
            out = dpr_amd.raster_smooth_bodies(grid, *args, algo=algo)
            assert out.shape == grid + (3,) and out.dtype == tdt
            for b in range(3):
                assert_close(out[..., b], c["out"][..., b].astype(npdt), tol(npdt, "out"), f"{grid} {algo} plane {b}")
        g = grid_to_dev(c["g"].astype(npdt), dev)
        for algo in ("atomic", "auto"):
            pb = dpr_amd.raster_pullback_smooth_bodies_(g, *args, algo=algo)
            assert pb.rotation.shape == (3, 3, n_out, n_in) and pb.translation.shape == (3, 3, n_out)
            _check_pullback(pb, c["pb"], npdt, f"{grid} {algo} ")
            never = torch.as_tensor(np.flatnonzero(~acc.any(axis=0)), device=dev)
            assert len(never) > 0 and bool((pb.points[never] == 0).all()) and bool((pb.point_weight[never] == 0).all())
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.raster_pullback_smooth_bodies_(g, *args, algo="tiled")
        assert dpr_amd.resolve_algo_smooth_bodies("pullback", grid, 777, 3, 3, n_in) == "atomic"


# ------------------------------------------------------------------ 2. composition of the single-body operator
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_planes_and_gradients_are_the_pieces_of_the_subset_calls(dev, npdt, tdt, n_in, n_out):
    """With background 0, plane b is the sum over k of raster_smooth_ of subset k under pose (b, k); each gradient is
    the matching piece of raster_pullback_smooth_ of that subset."""
    c = _case(n_in, n_out, order="shuffled")
    pts, body, rot, trans, _bg, ow, pw = _args(c, dev, npdt)
    g = grid_to_dev(c["g"].astype(npdt), dev)
    outs = {a: dpr_amd.raster_smooth_bodies(c["grid"], pts, body, rot, trans, None, ow, pw, algo=a) for a in FWD}
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, pts, body, rot, trans, None, ow, pw)
    total = torch.zeros_like(outs["atomic"])
    d_ow = torch.zeros_like(pb.out_weight)
    for k in range(c["K"]):
        idx = torch.nonzero(body == k).flatten()
        sub = (pts[idx].contiguous(), rot[:, k].contiguous(), trans[:, k].contiguous(), None, ow, pw[idx].contiguous())
        total += dpr_amd.raster_smooth(c["grid"], *sub, algo="atomic")
        p1 = dpr_amd.raster_pullback_smooth_(g, *sub, algo="atomic")
        assert_close(pb.points[idx], p1.points.cpu().numpy(), tol(npdt, "points"), f"ds_dpoints of body {k}")
        assert_close(pb.point_weight[idx], p1.point_weight.cpu().numpy(), tol(npdt, "points"), f"ds_dpw of body {k}")
        for b in range(c["B"]):
            assert_close(pb.rotation[b, k], p1.rotation[b].cpu().numpy(), tol(npdt, "pose"), f"ds_drotation[{b}, {k}]")
            assert_close(pb.translation[b, k], p1.translation[b].cpu().numpy(), tol(npdt, "pose"),
                         f"ds_dtranslation[{b}, {k}]")
        assert_close(pb.background, p1.background.cpu().numpy(), tol(npdt, "pose"), "ds_dbackground")
        d_ow += p1.out_weight
    assert_close(pb.out_weight, d_ow.cpu().numpy(), tol(npdt, "pose"), "ds_dout_weight")
    for a in FWD:
        for b in range(c["B"]):
            assert_close(outs[a][..., b], total[..., b].cpu().numpy(), tol(npdt, "out"), f"{a} plane {b}")


# ------------------------------------------------------------------ 3. K = 1 is the smooth splat
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_one_body_is_raster_smooth(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out, sizes=(777,), seed=1)
    pts, body, rot, trans, bg, ow, pw = _args(c, dev, npdt)
    want = dpr_amd.raster_smooth(c["grid"], pts, rot[:, 0], trans[:, 0], bg, ow, pw, algo="atomic").cpu().numpy()
    for algo in FWD:
        out = dpr_amd.raster_smooth_bodies(c["grid"], pts, body, rot, trans, bg, ow, pw, algo=algo)
        assert_close(out, want, tol(npdt, "out"), algo)
        assert_close(out, c["out"].astype(npdt), tol(npdt, "out"), f"{algo} against the reference")
    # one image: one thread adds one pose's terms in k_smooth_bwd's order and stores them
    g1 = dpr_amd.to_grid_layout(grid_to_dev(c["g"].astype(npdt), dev)[..., :1])
    one = (pts, rot[:1, 0], trans[:1, 0], bg[:1], ow[:1], pw)
    p1 = dpr_amd.raster_pullback_smooth_(g1, *one, algo="atomic")
    pb = dpr_amd.raster_pullback_smooth_bodies_(g1, pts, body, rot[:1], trans[:1], bg[:1], ow[:1], pw, algo="atomic")
    torch.cuda.synchronize()
    assert float(p1.points.abs().max()) > 0
    assert torch.equal(pb.points, p1.points)
    assert torch.equal(pb.point_weight, p1.point_weight)


# ------------------------------------------------------------------ 4. bodies out of range
@pytest.mark.parametrize("body_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_bodies_out_of_range_are_dropped(dev, body_dtype, npdt, tdt, n_in, n_out):
    """-1, K and 2^31 - 1 (int64: also +-2^40): those points deposit nothing, have exact-zero gradients, and the
    result equals the call without them."""
    c = _case(n_in, n_out, order="shuffled")
    K = c["K"]
    bad = np.arange(100, 130)  # (the cloud is shuffled: points of every body)
    body = np.array(c["body"])
    body[bad] = np.resize([-1, K, 2**31 - 1], 30)
    if body_dtype == torch.int64:
        body[bad[:4]] = (2**40, -(2**40), 2**40 + 1, -(2**40) + 2)
    keep = np.setdiff1d(np.arange(c["P"]), bad)
    args = _args(c, dev, npdt)
    args[1] = torch.as_tensor(body, device=dev).to(body_dtype)
    rest = [args[0][keep].contiguous(), args[1][keep].contiguous(), *args[2:6], args[6][keep].contiguous()]
    want = ref.raster(c["grid"], c["points"][keep], body[keep], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"][keep])
    for algo in FWD:
        out = dpr_amd.raster_smooth_bodies(c["grid"], *args, algo=algo)
        assert bool(torch.isfinite(out).all())
        assert_close(out, want.astype(npdt), tol(npdt, "out"), f"{algo} against the reference without them")
        without = dpr_amd.raster_smooth_bodies(c["grid"], *rest, algo=algo)
        assert_close(out, without.cpu().numpy(), tol(npdt, "out"), f"{algo} against the call without them")
    g = grid_to_dev(c["g"].astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, *args)
    pr = dpr_amd.raster_pullback_smooth_bodies_(g, *rest)
    assert bool((pb.points[bad] == 0).all()) and bool((pb.point_weight[bad] == 0).all())
    assert_close(pb.points[keep], pr.points.cpu().numpy(), tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight[keep], pr.point_weight.cpu().numpy(), tol(npdt, "points"), "ds_dpoint_weight")
    for name in ("rotation", "translation", "background", "out_weight"):
        assert_close(getattr(pb, name), getattr(pr, name).cpu().numpy(), tol(npdt, "pose"), name)
    wpb = ref.raster_pullback(c["g"], c["points"][keep], body[keep], c["rot"], c["trans"], c["ow"], c["pw"][keep])
    _check_pullback(pr, wpb, npdt, "without them ")


# ------------------------------------------------------------------ 5. a body without points
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_body_without_points_gets_exact_zeros(dev, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out, sizes=(300, 200, 0, 277), seed=2)
    assert c["K"] == 4 and 2 not in c["body"]
    args = _args(c, dev, npdt)
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
    d_rot, d_trans = nan(3, 4, n_in, n_out).transpose(-1, -2), nan(3, 4, n_out)
    pb = dpr_amd.raster_pullback_smooth_bodies_(grid_to_dev(c["g"].astype(npdt), dev), *args, ds_drotation=d_rot,
                                                ds_dtranslation=d_trans)
    assert pb.translation is d_trans and pb.rotation.data_ptr() == d_rot.data_ptr()
    assert bool((pb.rotation[:, 2] == 0).all()) and bool((pb.translation[:, 2] == 0).all())
    _check_pullback(pb, c["pb"], npdt)
    for algo in FWD:
        assert_close(dpr_amd.raster_smooth_bodies(c["grid"], *args, algo=algo), c["out"].astype(npdt),
                     tol(npdt, "out"), algo)


# ------------------------------------------------------------------ 6. wave and block mixes in the pullback
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_wave_and_block_mixes(dev, B, order, npdt, tdt, n_in, n_out):
    """P = 640 sorted with body sizes 256, 64, 64, 100, 156: block 0 holds one body (wave -> block -> one atomic);
    block 1 holds waves of one body each in a mixed block (bodies 1, 2) and mixed waves (3 into 4); block 2 is a
    partial block.  Shuffled: every wave walks five bodies.  B = 1: one launch, plain stores of the point gradients;
    B = 3: three slices, atomics onto zeroed buffers."""
    c = _case(n_in, n_out, sizes=MIX, B=B, order=order, seed=3)
    if order == "sorted":
        per_wave = [len(np.unique(c["body"][i:i + 64])) for i in range(0, 640, 64)]
        assert len(np.unique(c["body"][:256])) == 1 and per_wave[4] == 1 and per_wave[5] == 1 and 2 in per_wave[6:]
    else:
        assert min(len(np.unique(c["body"][i:i + 64])) for i in range(0, 640, 64)) == 5
    args = _args(c, dev, npdt)
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
    pb = dpr_amd.raster_pullback_smooth_bodies_(grid_to_dev(c["g"].astype(npdt), dev), *args,
                                                ds_dpoints=nan(640, n_in), ds_dpoint_weight=nan(640))
    _check_pullback(pb, c["pb"], npdt, f"{order} B={B} ")
    for algo in FWD:
        assert_close(dpr_amd.raster_smooth_bodies(c["grid"], *args, algo=algo), c["out"].astype(npdt),
                     tol(npdt, "out"), algo)


# ------------------------------------------------------------------ 7. groups of images
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_groups_of_images(dev, group, npdt, tdt, n_in, n_out):
    """B = 5: max_pose_group 1 (image by image), 2 (groups of 2 + 2 + 1) and 0 (all five images in one group)."""
    c = _case(n_in, n_out, sizes=(100, 100, 100), B=5, order="shuffled", seed=4)
    args = _args(c, dev, npdt)
    out = dpr_amd.raster_smooth_bodies(c["grid"], *args, algo="tiled", max_pose_group=group)
    for b in range(5):
        assert_close(out[..., b], c["out"][..., b].astype(npdt), tol(npdt, "out"), f"group {group} plane {b}")
    # in place, onto a buffer full of NaN
    buf = torch.full_like(out, float("nan"))
    assert dpr_amd.raster_smooth_bodies_(buf, *args, algo="tiled", max_pose_group=group) is buf
    assert bool(torch.isfinite(buf).all())
    assert_close(buf, c["out"].astype(npdt), tol(npdt, "out"), f"group {group} in place")
    with pytest.raises(ValueError):
        dpr_amd.raster_smooth_bodies(c["grid"], *args, algo="tiled", max_pose_group=17)


# ------------------------------------------------------------------ 8. two bodies on one cell
@pytest.mark.parametrize("algo", FWD)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_two_bodies_whose_poses_put_their_points_into_the_same_cell(dev, algo, npdt, tdt, n_in, n_out):
    """Body 0 under the identity and body 1 under a shift that moves its point onto body 0's: the 3^N cells hold the
    sum of the two deposits."""
    grid = GRIDS[n_out]
    eye = np.eye(n_out, n_in)
    p0 = np.full(n_in, 0.0625)
    shift = np.array([0.25, -0.5, 0.125])[:n_out]
    p1 = p0.copy()
    p1[:n_out] -= shift
    pts = np.stack([p0, p1])
    rot = np.stack([eye, eye])[None]
    trans = np.stack([np.zeros(n_out), shift])[None]
    pw = np.array([0.75, 1.5])
    body = torch.tensor([0, 1], device=dev)
    out = dpr_amd.raster_smooth_bodies(grid, T(pts.astype(npdt), dev), body, T(rot.astype(npdt), dev),
                                       T(trans.astype(npdt), dev), None, None, T(pw.astype(npdt), dev), algo=algo)
    one = dpr_amd.raster_smooth(grid, T(p0[None].astype(npdt), dev), T(eye[None].astype(npdt), dev),
                                T(np.zeros((1, n_out), npdt), dev), None, None, T(np.array([2.25], npdt), dev),
                                algo="atomic")
    assert int((one != 0).sum()) == 3 ** n_out
    assert_close(out, one.cpu().numpy(), tol(npdt, "out"), "the sum of the two deposits")
    assert abs(float(out.double().sum()) - 2.25) <= tol(npdt, "out") * 2.25


# ------------------------------------------------------------------ 9. edge shapes
@pytest.mark.parametrize("algo", FWD)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_one_point_no_images_and_the_single_image_form(dev, algo, npdt, tdt, n_in, n_out):
    c = _case(n_in, n_out)
    grid, B, K = c["grid"], c["B"], c["K"]
    pts, body, rot, trans, bg, ow, pw = _args(c, dev, npdt)
    g = grid_to_dev(c["g"].astype(npdt), dev)
    # P = 0: the background, zero pose gradients, the grid sum
    none = (pts[:0], body[:0], rot, trans, bg, ow, pw[:0])
    out = dpr_amd.raster_smooth_bodies(grid, *none, algo=algo)
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(c["bg"].astype(npdt), grid + (B,)))
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, *none)
    assert pb.points.shape == (0, n_in) and pb.point_weight.shape == (0,)
    assert bool((pb.rotation == 0).all()) and bool((pb.translation == 0).all()) and bool((pb.out_weight == 0).all())
    assert_close(pb.background, c["g"].reshape(-1, B).sum(axis=0).astype(npdt), tol(npdt, "pose"), "P=0 ds_dbg")
    # P = 1 (an accepted point of body 1)
    i = int(np.flatnonzero((c["body"] == 1) & _accepted(c).all(axis=0))[0])
    sl = slice(i, i + 1)
    want = ref.raster(grid, c["points"][sl], c["body"][sl], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"][sl])
    wpb = ref.raster_pullback(c["g"], c["points"][sl], c["body"][sl], c["rot"], c["trans"], c["ow"], c["pw"][sl])
    one = (pts[sl].contiguous(), body[sl].contiguous(), rot, trans, bg, ow, pw[sl].contiguous())
    assert_close(dpr_amd.raster_smooth_bodies(grid, *one, algo=algo), want.astype(npdt), tol(npdt, "out"), "P=1")
    pb1 = dpr_amd.raster_pullback_smooth_bodies_(g, *one)
    _check_pullback(pb1, wpb, npdt, "P=1 ")
    assert bool((pb1.rotation[:, [0, 2]] == 0).all())
    # B = 0: empty images and pose gradients, zero point gradients
    e = lambda *s: torch.zeros(s, dtype=tdt, device=dev)
    out = dpr_amd.raster_smooth_bodies(grid, pts, body, e(0, K, n_out, n_in), e(0, K, n_out), algo=algo)
    assert out.shape == grid + (0,)
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
    pb = dpr_amd.raster_pullback_smooth_bodies_(dpr_amd.empty_grid(grid, 0, tdt, dev), pts, body,
                                                e(0, K, n_out, n_in), e(0, K, n_out), ds_dpoints=nan(c["P"], n_in),
                                                ds_dpoint_weight=nan(c["P"]))
    assert pb.rotation.shape == (0, K, n_out, n_in) and pb.translation.shape == (0, K, n_out)
    assert bool((pb.points == 0).all()) and bool((pb.point_weight == 0).all())
    # the single-image form: no B axis anywhere in the results
    b = 1
    out1 = dpr_amd.raster_smooth_bodies(grid, pts, body, rot[b], trans[b], float(c["bg"][b]), float(c["ow"][b]), pw,
                                        algo=algo)
    assert out1.shape == grid
    assert_close(out1, c["out"][..., b].astype(npdt), tol(npdt, "out"), "single image")
    s = dpr_amd.raster_pullback_smooth_bodies_(g[..., b].contiguous(), pts, body, rot[b], trans[b], float(c["bg"][b]),
                                               float(c["ow"][b]), pw)
    assert s.rotation.shape == (K, n_out, n_in) and s.translation.shape == (K, n_out)
    assert s.background.shape == () and s.out_weight.shape == () and s.points.shape == (c["P"], n_in)
    want1 = ref.raster_pullback(c["g"][..., b:b + 1], c["points"], c["body"], c["rot"][b:b + 1], c["trans"][b:b + 1],
                                c["ow"][b:b + 1], c["pw"])
    _check_pullback((s.points, s.rotation[None], s.translation[None], s.background[None], s.out_weight[None],
                     s.point_weight), want1, npdt, "single image ")


def test_pullback_without_the_point_weight_gradient(dev):
    c = _case(3, 3)
    args = _args(c, dev, np.float32)
    g = grid_to_dev(c["g"].astype(np.float32), dev)
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, *args, point_weight_grad=False)
    assert pb.point_weight is None
    _check_pullback(pb, c["pb"], np.float32, "no pw grad ")
    with pytest.raises(ValueError):
        dpr_amd.raster_pullback_smooth_bodies_(g, *args, point_weight_grad=False,
                                               ds_dpoint_weight=torch.empty(c["P"], device=dev))


# ------------------------------------------------------------------ 10. the exact derivative, fp64
@pytest.mark.parametrize("algo", FWD)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, algo, n_in, n_out):
    """raster_smooth_bodies_ad in fp64 on an 8^N grid with 2 images, 3 bodies and 12 points: central differences with
    h = 1e-6 of sum(out * g) in all six arguments, within 1e-6 * max|gradient| (the shape and the bound of
    tests/test_smooth_bodies_reference.py).  A forward on "tiled" differentiates on "auto"."""
    rng = np.random.default_rng(11)
    nb, K, npts, grid = 2, 3, 12, (8,) * n_out
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(npts, n_in)), rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out),
            rng.normal(size=nb), rng.uniform(0.5, 1.5, size=nb), rng.uniform(0.5, 1.5, size=npts)]
    body = torch.as_tensor(np.arange(npts) % K, device=dev)
    g = grid_to_dev(rng.normal(size=grid + (nb,)), dev)
    xs = [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    out = dpr_amd.raster_smooth_bodies_ad(grid, xs[0], body, *xs[1:], algo=algo)
    (out * g).sum().backward()
    grads = [x.grad.cpu().numpy() for x in xs]
    scale = max(np.abs(a).max() for a in grads)
    h = 1e-6
    with torch.no_grad():
        loss = lambda: float((dpr_amd.raster_smooth_bodies(grid, xs[0], body, *xs[1:], algo=algo) * g).sum())
        for name, x, ga in zip(FIELDS, xs, grads):
            flat = x.view(-1)
            fd = np.zeros(flat.numel())
            for i in range(flat.numel()):
                keep = float(flat[i])
                flat[i] = keep + h
                up = loss()
                flat[i] = keep - h
                dn = loss()
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd.reshape(ga.shape) - ga).max()
            assert err <= 1e-6 * scale, (name, err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_gradient_is_continuous_across_a_cell_face(dev, n_in, n_out):
    """Every point of body 1 sits 1e-9 cells either side of a cell face of axis 0 in image 1 (fp64): the gradients of
    the two calls differ by less than 1e-6 * max|gradient|."""
    rng = np.random.default_rng(5)
    grid, nb, K, per = (8,) * n_out, 3, 3, 6
    g = grid_to_dev(rng.normal(size=grid + (nb,)), dev)
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    rot, trans = rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out)
    pts = np.concatenate([_cloud(rng, grid, rot[1, k], trans[1, k], n_in, per, lo=1.0, hi=-1.0) for k in range(K)])
    body = np.repeat(np.arange(K), per)
    face = np.array([2, 3, 4, 5, 6, 3], dtype=np.float64)
    base = rng.uniform(1, 7, size=(per, n_out))
    sides = []
    for eps in (-1e-9, 1e-9):
        coord = base.copy()
        coord[:, 0] = face + eps
        p = pts.copy()
        p[body == 1] = ((-1 + 2 * coord / 8) - trans[1, 1]) @ rot[1, 1]
        sides.append(p)
    lo, hi = sides
    assert np.all(np.floor(_coords(grid, lo[body == 1], rot[1, 1], trans[1, 1])[:, 0]) + 1
                  == np.floor(_coords(grid, hi[body == 1], rot[1, 1], trans[1, 1])[:, 0]))
    tb = torch.as_tensor(body, device=dev)
    run = lambda p: dpr_amd.raster_pullback_smooth_bodies_(g, T(p, dev), tb, T(rot, dev), T(trans, dev))
    pa, pb = run(lo), run(hi)
    scale = max(float(a.abs().max()) for a in pa)
    for a, b in zip(pa, pb):
        assert float((a - b).abs().max()) < 1e-6 * scale
