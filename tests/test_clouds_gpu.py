"""Per-pose point clouds on the GPU (dpr_raster_clouds_ex_*, dpr_raster_pullback_clouds_ex_*).

The ground truth is the oracle composed per pose: plane b and the gradients of pose b are oracle.raster /
oracle.raster_pullback with B = 1 on (cloud b, pose b).  Tolerances are those of tests/test_parity_gpu.py."""
import numpy as np
import pytest
import torch

import dpr_amd
from oracle import oracle
from tests import data as D

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
ALL_ALGO_PAIRS = [(2, 2), (3, 3), (3, 2)]
CASES = [(a, i, o) for a in ("atomic", "tiled", "chunked") for (i, o) in ALL_ALGO_PAIRS] + \
    [("atomic", i, o) for (i, o) in ((1, 1), (2, 3), (4, 2), (4, 4))]
NAMES = ("points", "rotation", "translation", "background", "out_weight", "point_weight")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def tol(npdt, kind):
    if npdt == np.float64:
        return 1e-10
    return {"out": 5e-5, "points": 1e-4, "pose": 1e-3}[kind]


def assert_close(actual, expected, rtol, what=""):
    a = actual.detach().cpu().numpy() if isinstance(actual, torch.Tensor) else np.asarray(actual)
    e = np.asarray(expected)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    na, ne = np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel())
    err = np.linalg.norm((a.astype(np.float64) - e.astype(np.float64)).ravel())
    assert err <= rtol * max(na, ne) + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{max(na, ne):.3e}"


def clouds(n_in, n_out, B, P, grid, seed=0, pad=True, faces=True):
    """B clouds of P points with a different spread per pose, a few points outside the grid, pose 0 mapping points
    onto cell faces, and (pad) uneven cloud sizes padded with zero weights."""
    rng = np.random.default_rng(seed)
    grid = tuple(grid)
    d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=seed)
    rot, trans = d.rotations.copy(), d.translations.copy()
    pts = np.empty((B, P, n_in))
    for b in range(B):
        pts[b] = (0.15 + 0.4 * rng.uniform()) * rng.normal(size=(P, n_in))
        pts[b, :P // 50] *= 6.0  # outside the grid
    # pose 0: an axis-aligned projection, and points whose coordinates are cell faces
    rot[0] = np.eye(n_out, n_in)
    trans[0] = 0.0
    k = min(P // 10, 64) if faces else 0
    for j in range(min(n_in, n_out)):
        pts[0, :k, j] = -1.0 + 2.0 * rng.integers(0, grid[j] + 1, size=k) / grid[j]
    pw = rng.uniform(0.5, 1.5, size=(B, P))
    if pad:
        for b in range(B):
            pw[b, P - (b * P) // (2 * B):] = 0.0
    bg = np.arange(1, B + 1, dtype=np.float64)
    ow = rng.uniform(1, 10, size=B)
    ds = rng.normal(size=grid + (B,))
    return dict(grid=grid, points=pts, rot=rot, trans=trans, pw=pw, bg=bg, ow=ow, ds=ds, B=B, P=P)


def on(dev, tdt, c):
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    t = {k: to(c[k]) for k in ("points", "rot", "trans", "pw", "bg", "ow")}
    t["ds"] = dpr_amd.to_grid_layout(to(c["ds"]))
    return t


def oracle_forward(c, npdt, b):
    return oracle.raster(c["grid"], c["points"][b], c["rot"][b:b + 1], c["trans"][b:b + 1], c["bg"][b:b + 1],
                         c["ow"][b:b + 1], c["pw"][b], dtype=npdt)[..., 0]


def oracle_pullback(c, npdt, b):
    return oracle.raster_pullback(c["ds"][..., b:b + 1], c["points"][b], c["rot"][b:b + 1], c["trans"][b:b + 1],
                                  c["ow"][b:b + 1], c["pw"][b], dtype=npdt)


def check_against_oracle(c, out, pb, npdt, poses=None):
    poses = range(c["B"]) if poses is None else poses
    for b in poses:
        assert_close(out[..., b], oracle_forward(c, npdt, b), tol(npdt, "out"), f"out[.., {b}]")
        r = oracle_pullback(c, npdt, b)
        assert_close(pb.points[b], r.points, tol(npdt, "points"), f"ds_dpoints[{b}]")
        assert_close(pb.point_weight[b], r.point_weight, tol(npdt, "points"), f"ds_dpoint_weight[{b}]")
        assert_close(pb.rotation[b], r.rotation[0], tol(npdt, "pose"), f"ds_drotation[{b}]")
        assert_close(pb.translation[b], r.translation[0], tol(npdt, "pose"), f"ds_dtranslation[{b}]")
        assert_close(pb.background[b:b + 1], r.background, tol(npdt, "pose"), f"ds_dbackground[{b}]")
        assert_close(pb.out_weight[b:b + 1], r.out_weight, tol(npdt, "pose"), f"ds_dout_weight[{b}]")


def run(t, c, algo, **kw):
    out = dpr_amd.raster_clouds(c["grid"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"], algo=algo,
                                **kw)
    pb = dpr_amd.raster_pullback_clouds_(t["ds"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                         algo=algo)
    torch.cuda.synchronize()
    return out, pb


# ------------------------------------------------------------------ 1. every algorithm against the oracle
@pytest.mark.parametrize("algo,n_in,n_out", CASES)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_matches_the_oracle_composed_per_pose(dev, algo, n_in, n_out, npdt, tdt):
    c = clouds(n_in, n_out, B=5, P=1999, grid=(8,) * n_out if n_out == 4 else (16,) * n_out, seed=n_in * 10 + n_out)
    out, pb = run(on(dev, tdt, c), c, algo)
    assert out.shape == c["grid"] + (5,) and out.dtype == tdt
    check_against_oracle(c, out, pb, npdt)


# ------------------------------------------------------------------ 2. CHUNKED on grids of one tile and of several
@pytest.mark.parametrize("grid,n_in", [((64, 64), 3), ((200, 150), 3), ((200, 150), 2), ((40, 33, 20), 3),
                                       ((128, 128), 3)])
@pytest.mark.parametrize("P", [1500, 20000])  # one slice per (pose, tile) / several slices
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_tiles_and_slices(dev, grid, n_in, P, npdt, tdt):
    c = clouds(n_in, len(grid), B=3, P=P, grid=grid, seed=P + len(grid))
    out, pb = run(on(dev, tdt, c), c, "chunked")
    check_against_oracle(c, out, pb, npdt)


# ------------------------------------------------------------------ 3. bit-for-bit checks
@pytest.mark.parametrize("n_in,n_out", ALL_ALGO_PAIRS)
def test_tiled_planes_are_the_single_pose_tiled_calls(dev, n_in, n_out):
    c = clouds(n_in, n_out, B=3, P=4000, grid=(48,) * n_out, seed=5)  # (no tile split into parts)
    t = on(dev, torch.float32, c)
    out, pb = run(t, c, "tiled")
    for b in range(3):
        one = dpr_amd.raster(c["grid"], t["points"][b], t["rot"][b], t["trans"][b], t["bg"][b], t["ow"][b],
                             t["pw"][b], algo="tiled")
        p1 = dpr_amd.raster_pullback_(t["ds"][..., b], t["points"][b], t["rot"][b], t["trans"][b], t["bg"][b],
                                      t["ow"][b], t["pw"][b], algo="tiled")
        torch.cuda.synchronize()
        if n_out == 3:
            assert torch.equal(out[..., b], one), b
        else:  # (the single-pose tiled forward itself varies at rounding level run to run on small 2-D grids)
            d = (out[..., b].double() - one.double()).abs().max().item()
            assert d <= 4e-6 * one.double().abs().max().item(), b
        assert torch.equal(pb.points[b], p1.points), b
        assert torch.equal(pb.point_weight[b], p1.point_weight), b


@pytest.mark.parametrize("n_in,n_out", [(3, 2), (3, 3), (2, 2), (4, 4)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_atomic_pullback_of_one_pose_is_the_single_pose_atomic_pullback(dev, n_in, n_out, npdt, tdt):
    c = clouds(n_in, n_out, B=1, P=5000, grid=(8,) * n_out if n_out == 4 else (24,) * n_out, seed=3)
    t = on(dev, tdt, c)
    pb = dpr_amd.raster_pullback_clouds_(t["ds"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                         algo="atomic")
    p1 = dpr_amd.raster_pullback_(t["ds"], t["points"][0], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"][0],
                                  algo="atomic")
    torch.cuda.synchronize()
    assert torch.equal(pb.points[0], p1.points)
    assert torch.equal(pb.point_weight[0], p1.point_weight)


@pytest.mark.parametrize("grid,n_in", [((64, 64), 3), ((128, 128), 2), ((40, 33, 20), 3)])
def test_chunked_fp32_one_slice_is_exact_and_order_independent(dev, grid, n_in):
    c = clouds(n_in, len(grid), B=4, P=2000, grid=grid, seed=11)
    t = on(dev, torch.float32, c)
    out1 = dpr_amd.raster_clouds(grid, t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"], algo="chunked")
    out2 = dpr_amd.raster_clouds(grid, t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"], algo="chunked")
    perm = torch.stack([torch.randperm(c["P"], generator=torch.Generator().manual_seed(b)) for b in range(4)])
    perm = perm.to(dev)
    pts = torch.gather(t["points"], 1, perm[..., None].expand(-1, -1, n_in)).contiguous()
    pw = torch.gather(t["pw"], 1, perm).contiguous()
    out3 = dpr_amd.raster_clouds(grid, pts, t["rot"], t["trans"], t["bg"], t["ow"], pw, algo="chunked")
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    assert torch.equal(out1, out3)


@pytest.mark.parametrize("grid,n_in,P", [((64, 64), 3, 3000), ((200, 150), 2, 20000), ((40, 33, 20), 3, 20000)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_pullback_is_bit_reproducible(dev, grid, n_in, P, npdt, tdt):
    c = clouds(n_in, len(grid), B=3, P=P, grid=grid, seed=12)
    t = on(dev, tdt, c)
    a = dpr_amd.raster_pullback_clouds_(t["ds"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                        algo="chunked")
    b = dpr_amd.raster_pullback_clouds_(t["ds"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                        algo="chunked")
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, b):
        if name == "background":  # (grid_sum: one float atomic per block, rounding level with several blocks)
            assert_close(x, y.cpu().numpy(), 1e-12 if npdt == np.float64 else 1e-6, name)
        else:
            assert torch.equal(x, y), name


# ------------------------------------------------------------------ 4. coverage: every output fully overwritten
@pytest.mark.parametrize("algo,n_in,n_out", [("atomic", 3, 2), ("tiled", 3, 3), ("chunked", 3, 2),
                                             ("chunked", 3, 3), ("chunked", 2, 2), ("atomic", 2, 3)])
def test_outputs_prefilled_with_nan_are_overwritten(dev, algo, n_in, n_out):
    c = clouds(n_in, n_out, B=3, P=4000, grid=(200, 150) if n_out == 2 else (40, 33, 20), seed=13)
    t = on(dev, torch.float32, c)
    B, P = 3, 4000
    out = dpr_amd.empty_grid(c["grid"], B, torch.float32, dev).fill_(float("nan"))
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    bufs = dict(ds_dpoints=nan(B, P, n_in), ds_drotation=nan(B, n_in, n_out).transpose(1, 2),
                ds_dtranslation=nan(B, n_out), ds_dbackground=nan(B), ds_dout_weight=nan(B),
                ds_dpoint_weight=nan(B, P))
    dpr_amd.raster_clouds_(out, t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"], algo=algo)
    pb = dpr_amd.raster_pullback_clouds_(t["ds"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                         algo=algo, **bufs)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    for name, x in zip(NAMES, pb):
        assert not torch.isnan(x).any(), name
    assert pb.points is bufs["ds_dpoints"] and pb.point_weight is bufs["ds_dpoint_weight"]
    # padded (zero-weight) points: no position gradient
    zero = t["pw"] == 0
    assert zero.any() and (pb.points[zero] == 0).all()


# ------------------------------------------------------------------ 5. consistency with the shared-cloud entry points
@pytest.mark.parametrize("algo", ["atomic", "tiled", "chunked"])
def test_copies_of_one_cloud_match_shared_cloud_raster(dev, algo):
    d = D.make(n_points=6000, n_in=3, n_out=2, batch=5, grid_n=64, seed=14, dtype=np.float32)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    pts, R, tr, bg, ow, pw = map(to, (d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                                      d.point_weights))
    ds = dpr_amd.to_grid_layout(to(d.ds_dout))
    many = pts[None].expand(5, -1, -1).contiguous()
    out = dpr_amd.raster_clouds(d.grid, many, R, tr, bg, ow, pw, algo=algo)
    ref = dpr_amd.raster(d.grid, pts, R, tr, bg, ow, pw, algo="atomic")
    pb = dpr_amd.raster_pullback_clouds_(ds, many, R, tr, bg, ow, pw, algo=algo)
    pr = dpr_amd.raster_pullback_(ds, pts, R, tr, bg, ow, pw, algo="atomic")
    torch.cuda.synchronize()
    assert_close(out, ref.cpu().numpy(), 5e-5, "out")
    assert_close(pb.points.sum(0), pr.points.cpu().numpy(), 1e-4, "ds_dpoints")
    assert pb.point_weight.shape == (6000,)  # a (P,) point_weight gets the sum over poses
    assert_close(pb.point_weight, pr.point_weight.cpu().numpy(), 1e-4, "ds_dpoint_weight")
    for name in ("rotation", "translation", "background", "out_weight"):
        assert_close(getattr(pb, name), getattr(pr, name).cpu().numpy(), 1e-3, name)


# ------------------------------------------------------------------ 6. autograd
@pytest.mark.parametrize("algo", ["atomic", "chunked"])
@pytest.mark.parametrize("shared_pw", [False, True])
def test_gradcheck_raster_clouds_ad(dev, algo, shared_pw):
    c = clouds(3, 2, B=2, P=30, grid=(8, 8), seed=15, pad=False, faces=False)  # (no kinks under the differences)
    t = on(dev, torch.float64, c)
    pw = t["pw"][0] if shared_pw else t["pw"]
    args = [t["points"].clone().requires_grad_(), t["rot"].clone().requires_grad_(),
            t["trans"].clone().requires_grad_(), t["bg"].clone().requires_grad_(), t["ow"].clone().requires_grad_(),
            pw.clone().requires_grad_()]
    fn = lambda pts, R, tr, bg, ow, w: dpr_amd.raster_clouds_ad(c["grid"], pts, R, tr, bg, ow, w, algo=algo)
    assert torch.autograd.gradcheck(fn, tuple(args), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=1e-12)


# ------------------------------------------------------------------ 7. a full-size minibatch through AUTO
def test_flexible_minibatch_through_auto(dev):
    c = clouds(3, 2, B=256, P=20000, grid=(128, 128), seed=16)
    t = on(dev, torch.float32, c)
    out, pb = run(t, c, "auto")
    check_against_oracle(c, out, pb, np.float32, poses=(0, 1, 97, 255))
