"""Multi-channel rasterisation on the GPU (dpr_raster_channels_ex_*, dpr_raster_pullback_channels_ex_*).

Everything rests on the per-channel decomposition of include/dpr.h (MULTI-CHANNEL): plane c of the forward is
the single-channel `raster` of point_weight[:, c] / background[..., c]; ds_dpoints and the per-pose sums of the
pullback are the sums over c of the single-channel results, ds_dpoint_weight[:, c] / ds_dbackground[..., c]
the single-channel results of channel c.  Tolerances are those of tests/test_parity_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from oracle import oracle
from tests import data as D

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]


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
    e = expected.detach().cpu().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    na, ne = np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel())
    err = np.linalg.norm((a.astype(np.float64) - e.astype(np.float64)).ravel())
    assert err <= rtol * max(na, ne) + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{max(na, ne):.3e}"


def problem(dev, tdt, n_in, n_out, B, C, P=3000, grid_n=16, seed=0):
    """Single pose (B = None) or a batch; channel weights / backgrounds that differ per channel."""
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B or 1, grid_n=grid_n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    pw = rng.uniform(0.2, 1.0, size=(P, C)) * (1.0 + np.arange(C))
    bg = rng.uniform(-1, 1, size=(B or 1, C))
    ow = d.weights
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    p = dict(points=to(d.points), pw=to(pw), grid=d.grid)
    if B is None:
        p.update(rot=to(d.rotations[0]), trans=to(d.translations[0]), bg=to(bg[0]), ow=float(ow[0]))
    else:
        p.update(rot=to(d.rotations), trans=to(d.translations), bg=to(bg), ow=to(ow))
    return p


def plane(out, c, n_out):
    """out[.., c(, b)] as a tensor of the single-channel shape."""
    return out.select(n_out, c)


def single(p, c, algo):
    bg = p["bg"][..., c]
    bg = float(bg) if bg.ndim == 0 else bg
    return dpr_amd.raster(p["grid"], p["points"], p["rot"], p["trans"], bg, p["ow"],
                          p["pw"][:, c].contiguous(), algo=algo)


def oracle_plane(p, c, npdt):
    pts = p["points"].double().cpu().numpy()
    R = p["rot"].double().cpu().numpy()
    t = p["trans"].double().cpu().numpy()
    if R.ndim == 2:
        R, t = R[None], t[None]
    bg = p["bg"][..., c].double().cpu().numpy().reshape(-1)
    ow = np.asarray(p["ow"].double().cpu().numpy() if isinstance(p["ow"], torch.Tensor) else [p["ow"]]).reshape(-1)
    out = oracle.raster(p["grid"], pts, R, t, bg, ow, p["pw"][:, c].double().cpu().numpy(), dtype=npdt)
    return out if p["rot"].ndim == 3 else out[..., 0]


# ------------------------------------------------------------------ 1. forward decomposition
FWD_CASES = [(algo, n_in, n_out) for algo in ("atomic", "tiled", "auto") for (n_in, n_out) in
             ((2, 2), (3, 3), (3, 2))] + [("atomic", 2, 3), ("atomic", 4, 4)]


@pytest.mark.parametrize("algo,n_in,n_out", FWD_CASES)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("C", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("B", [None, 4])
def test_forward_planes_are_single_channel_rasters(dev, algo, n_in, n_out, npdt, tdt, C, B):
    grid_n = 8 if n_out == 4 else 16
    p = problem(dev, tdt, n_in, n_out, B, C, P=2000, grid_n=grid_n, seed=C + n_in * 10 + n_out)
    out = dpr_amd.raster_channels(p["grid"], p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                  algo=algo)
    expect_shape = tuple(p["grid"]) + (C,) + (() if B is None else (B,))
    assert tuple(out.shape) == expect_shape
    # memory: a contiguous (B, C, n_N, .., n_1) tensor
    assert out.permute(*reversed(range(out.ndim))).is_contiguous()
    torch.cuda.synchronize()
    for c in range(C):
        ref = single(p, c, algo)
        got = plane(out, c, n_out)
        assert_close(got, ref, tol(npdt, "out"), f"plane {c} vs single-channel")
        if algo == "tiled" and npdt == np.float32 and B is None:
            assert torch.equal(got, ref), f"plane {c}: not bit-identical to the single-channel TILED call"
        assert_close(got, oracle_plane(p, c, npdt), tol(npdt, "out"), f"plane {c} vs oracle")


# ------------------------------------------------------------------ 2. bit-equality under fp32 TILED
def _bit_equal_or_rounding(got, ref, rerun, what):
    """Bit-equal to the single-channel call wherever that call reproduces itself bit for bit; a call whose
    split tiles vary run to run (include/dpr.h, SUMMATION ORDER) is held to rounding level instead."""
    if torch.equal(ref, rerun):
        assert torch.equal(got, ref), f"{what}: not bit-identical (single-channel call is reproducible)"
    else:
        d = (got.double() - ref.double()).abs().max().item()
        assert d <= 4e-6 * ref.double().abs().max().item(), f"{what}: {d}"


@pytest.mark.parametrize("case", ["clustered", "full_c3"])
def test_tiled_fp32_planes_bit_identical(dev, case):
    rng = np.random.default_rng(5)
    if case == "clustered":  # most of the cloud in a few tiles: heavy tiles split into parts
        P, grid = 400_000, (64, 64, 64)
        pts = np.concatenate([0.02 * rng.normal(size=(P // 2, 3)),
                              0.4 * rng.normal(size=(P - P // 2, 3))])
    else:
        P, grid = 10_000_000, (256, 256, 256)
        pts = 0.4 * rng.normal(size=(P, 3))
    C = 3
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    pts_t = to(pts)
    R = to(D.random_rotations(rng, 1)[0])
    t = to(0.05 * rng.normal(size=3))
    pw = to(rng.uniform(0.1, 1.0, size=(P, C)))
    bg = to([0.5, -1.0, 2.0])
    out = dpr_amd.raster_channels(grid, pts_t, R, t, pw, bg, 1.7, algo="tiled")
    for c in range(C):
        args = (grid, pts_t, R, t, float(bg[c]), 1.7, pw[:, c].contiguous())
        ref = dpr_amd.raster(*args, algo="tiled")
        rerun = dpr_amd.raster(*args, algo="tiled")
        _bit_equal_or_rounding(plane(out, c, 3), ref, rerun, f"{case} plane {c}")
    # default weights: every plane is the single-channel default-weight call
    ones = torch.ones_like(pw)
    out1 = dpr_amd.raster_channels(grid, pts_t, R, t, ones, bg, 1.7, algo="tiled")
    ref = dpr_amd.raster(grid, pts_t, R, t, float(bg[1]), 1.7, ones[:, 1].contiguous(), algo="tiled")
    rerun = dpr_amd.raster(grid, pts_t, R, t, float(bg[1]), 1.7, ones[:, 1].contiguous(), algo="tiled")
    _bit_equal_or_rounding(plane(out1, 1, 3), ref, rerun, f"{case} ones")


# ------------------------------------------------------------------ 3. per-channel range guard
def test_range_guard_is_per_channel(dev):
    """Channel 1's weights span 2^20 (its scope falls back to f64 atomics); channels 0 and 2 span 2^2 and
    keep their exact fixed-point sums, bit-identical to their single-channel calls."""
    rng = np.random.default_rng(11)
    P, grid = 300_000, (64, 64, 64)
    pts = 0.4 * rng.normal(size=(P, 3))
    pw = np.stack([rng.uniform(1, 4, P), 2.0 ** rng.uniform(-10, 10, P), rng.uniform(0.25, 1, P)], 1)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    R = D.random_rotations(rng, 1)
    t = 0.05 * rng.normal(size=(1, 3))
    out = dpr_amd.raster_channels(grid, to(pts), to(R[0]), to(t[0]), to(pw), None, 1.0, algo="tiled")
    for c in (0, 2):
        args = (grid, to(pts), to(R[0]), to(t[0]), None, 1.0, to(pw[:, c]))
        ref = dpr_amd.raster(*args, algo="tiled")
        rerun = dpr_amd.raster(*args, algo="tiled")
        _bit_equal_or_rounding(plane(out, c, 3), ref, rerun, f"guard plane {c}")
    p32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    expect = oracle.raster(grid, p32(pts), p32(R), p32(t), None, np.ones(1), p32(pw[:, 1]), dtype=np.float64)[..., 0]
    assert_close(plane(out, 1, 3), expect, 5e-5, "wide-range channel vs fp64 oracle")
    # cells holding only light contributions keep their relative precision (the guard's promise; the fp32
    # oracle makes the same cell choices)
    exp32 = oracle.raster(grid, p32(pts), p32(R), p32(t), None, np.ones(1), p32(pw[:, 1]), dtype=np.float32)[..., 0]
    got = plane(out, 1, 3).cpu().numpy()
    small = (exp32 > 0) & (exp32 < 1e-3 * exp32.max())
    assert small.sum() > 100
    assert_close(got[small], exp32[small], 1e-4, "light cells of the wide-range channel")


# ------------------------------------------------------------------ 4. pullback decomposition
PB_SHAPES = [(2, 2), (3, 3), (3, 2), (2, 3), (4, 4)]


@pytest.mark.parametrize("n_in,n_out", PB_SHAPES)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("C", [1, 3, 5, 16])
@pytest.mark.parametrize("B", [None, 4])
@pytest.mark.parametrize("pw_grad", [True, False])
def test_pullback_decomposes_over_channels(dev, n_in, n_out, npdt, tdt, C, B, pw_grad):
    grid_n = 8 if n_out == 4 else 16
    p = problem(dev, tdt, n_in, n_out, B, C, P=2000, grid_n=grid_n, seed=3 * C + n_in)
    rng = np.random.default_rng(C)
    shape = tuple(p["grid"]) + (C,) + (() if B is None else (B,))
    g = dpr_amd.empty_channel_grid(p["grid"], C, B, tdt, dev)
    g.copy_(torch.as_tensor(rng.normal(size=shape), device=dev))
    pb = dpr_amd.raster_pullback_channels_(g, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                           point_weight_grad=pw_grad)
    sums = None
    for c in range(C):
        bg = p["bg"][..., c]
        r = dpr_amd.raster_pullback_(g.select(n_out, c), p["points"], p["rot"], p["trans"],
                                     float(bg) if bg.ndim == 0 else bg, p["ow"], p["pw"][:, c].contiguous(),
                                     algo="atomic")
        if pw_grad:
            assert_close(pb.point_weight[:, c], r.point_weight, tol(npdt, "points"), f"ds_dpoint_weight[:, {c}]")
        assert_close(pb.background[..., c], r.background, tol(npdt, "pose"), f"ds_dbackground[.., {c}]")
        parts = (r.points, r.rotation, r.translation, r.out_weight)
        sums = [x.double() for x in parts] if sums is None else [s + x.double() for s, x in zip(sums, parts)]
    if not pw_grad:
        assert pb.point_weight is None
    assert_close(pb.points, sums[0], tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.rotation, sums[1], tol(npdt, "pose"), "ds_drotation")
    assert_close(pb.translation, sums[2], tol(npdt, "pose"), "ds_dtranslation")
    assert_close(pb.out_weight, sums[3], tol(npdt, "pose"), "ds_dout_weight")


# ------------------------------------------------------------------ 5. autograd
def test_gradcheck_raster_channels_ad(dev):
    p = problem(dev, torch.float64, 3, 2, 2, 3, P=40, grid_n=8, seed=4)
    args = [p["points"].clone().requires_grad_(), p["rot"].clone().requires_grad_(),
            p["trans"].clone().requires_grad_(), p["pw"].clone().requires_grad_(),
            p["bg"].clone().requires_grad_(), p["ow"].clone().requires_grad_()]
    fn = lambda pts, R, t, pw, bg, ow: dpr_amd.raster_channels_ad(p["grid"], pts, R, t, pw, bg, ow)
    assert torch.autograd.gradcheck(fn, tuple(args), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=1e-12)


def test_ds_dpoints_central_differences(dev):
    p = problem(dev, torch.float64, 3, 3, None, 3, P=200, grid_n=16, seed=9)
    rng = np.random.default_rng(9)
    g = dpr_amd.empty_channel_grid(p["grid"], 3, None, torch.float64, dev)
    g.copy_(torch.as_tensor(rng.normal(size=tuple(p["grid"]) + (3,)), device=dev))
    pb = dpr_amd.raster_pullback_channels_(g, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"])

    def loss(pts):
        out = dpr_amd.raster_channels(p["grid"], pts, p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                      algo="atomic")
        return float((out * g).sum())

    h = 1e-6
    for i in range(0, 200, 23):
        for j in range(3):
            e = torch.zeros_like(p["points"])
            e[i, j] = h
            fd = (loss(p["points"] + e) - loss(p["points"] - e)) / (2 * h)
            assert abs(fd - float(pb.points[i, j])) <= 1e-5 * max(1.0, abs(fd)), (i, j, fd, float(pb.points[i, j]))


# ------------------------------------------------------------------ 6. C = 1 is the existing API
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [None, 4])
def test_one_channel_equals_the_existing_api(dev, npdt, tdt, B):
    p = problem(dev, tdt, 3, 3, B, 1, P=5000, grid_n=24, seed=21)
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_channels(p["grid"], p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                      algo=algo)
        ref = single(p, 0, algo)
        if algo == "tiled" and npdt == np.float32 and B is None:  # exact fixed-point sums: deterministic
            assert torch.equal(plane(out, 0, 3), ref)
        else:
            assert_close(plane(out, 0, 3), ref, tol(npdt, "out"), algo)
    g = dpr_amd.empty_channel_grid(p["grid"], 1, B, tdt, dev)
    g.copy_(torch.as_tensor(np.random.default_rng(2).normal(size=tuple(g.shape)), device=dev))
    pb = dpr_amd.raster_pullback_channels_(g, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"])
    bg = p["bg"][..., 0]
    r = dpr_amd.raster_pullback_(g.select(3, 0), p["points"], p["rot"], p["trans"],
                                 float(bg) if bg.ndim == 0 else bg, p["ow"], p["pw"][:, 0].contiguous(),
                                 algo="atomic")
    # the direct pullback stores a point's gradients from one thread, poses in index order: deterministic,
    # and C = 1 runs the single-channel arithmetic -- unless poses were sliced over blocks (then atomics)
    if B is None:
        assert torch.equal(pb.points, r.points)
        assert torch.equal(pb.point_weight[:, 0], r.point_weight)
    assert_close(pb.points, r.points, tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight[:, 0], r.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
    for name in ("rotation", "translation", "out_weight"):
        assert_close(getattr(pb, name), getattr(r, name), tol(npdt, "pose"), name)
    assert_close(pb.background[..., 0], r.background, tol(npdt, "pose"), "background")


# ------------------------------------------------------------------ 7. errors
def test_errors_leave_outputs_untouched(dev):
    p = problem(dev, torch.float32, 3, 3, 2, 3, P=500, grid_n=8, seed=1)
    out = dpr_amd.empty_channel_grid(p["grid"], 3, 2, torch.float32, dev)
    out.fill_(7.0)
    sentinel = out.clone()
    L = dpr_amd.lib()
    g = np.asarray(p["grid"], dtype=np.int64)
    gp = g.ctypes.data_as(ctypes.c_void_p)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rot_cm = p["rot"].transpose(1, 2).contiguous()
    call = lambda algo, C, n_in=3, n_out=3: L.dpr_raster_channels_ex_f32(
        stream, algo, 0, n_in, n_out, gp, 500, 2, C, ptr(out), ptr(p["points"]), ptr(rot_cm), ptr(p["trans"]),
        ptr(p["bg"]), ptr(p["ow"]), ptr(p["pw"]), None, 0)
    assert call(_lib.ALGO_AUTO, 0) == _lib.ERR_INVALID_ARG
    assert call(_lib.ALGO_ATOMIC, 17) == _lib.ERR_INVALID_ARG
    assert call(_lib.ALGO_CHUNKED, 3) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(_lib.ALGO_TILED, 3, n_in=2) == _lib.ERR_UNSUPPORTED_ALGO  # (2,3): direct kernels only
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel)
    with pytest.raises(dpr_amd.DimensionMismatch):  # a (P,) point_weight
        dpr_amd.raster_channels_(out, p["points"], p["rot"], p["trans"], p["pw"][:, 0].contiguous(), None,
                                 p["ow"])
    with pytest.raises(dpr_amd.DimensionMismatch):  # background (B,) instead of (B, C)
        dpr_amd.raster_channels_(out, p["points"], p["rot"], p["trans"], p["pw"], p["bg"][:, 0].contiguous(),
                                 p["ow"])
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.raster_channels_(out, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"], algo="chunked")
    assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.raster_channels_(out, p["points"], p["rot"], p["trans"], torch.ones(500, 17, device=dev), None,
                                 p["ow"])
    assert e.value.code == _lib.ERR_INVALID_ARG
    q = problem(dev, torch.float32, 2, 3, 2, 3, P=500, grid_n=8, seed=1)
    out23 = dpr_amd.empty_channel_grid(q["grid"], 3, 2, torch.float32, dev).fill_(7.0)
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.raster_channels_(out23, q["points"], q["rot"], q["trans"], q["pw"], q["bg"], q["ow"], algo="tiled")
    assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    gb = dpr_amd.empty_channel_grid(p["grid"], 3, 2, torch.float32, dev).fill_(1.0)
    d_pts = torch.full((500, 3), 3.0, device=dev)
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.raster_pullback_channels_(gb, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                          ds_dpoints=d_pts, algo="tiled")
    assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel)
    assert bool((out23 == 7.0).all()) and bool((d_pts == 3.0).all())


@pytest.mark.parametrize("algo", [_lib.ALGO_ATOMIC, _lib.ALGO_TILED])
def test_null_point_weight_means_one_in_every_channel(dev, algo):
    p = problem(dev, torch.float32, 3, 3, 2, 3, P=4000, grid_n=16, seed=6)
    out = dpr_amd.empty_channel_grid(p["grid"], 3, 2, torch.float32, dev)
    g = np.asarray(p["grid"], dtype=np.int64)
    ws_n = dpr_amd.workspace_bytes_channels("raster", p["grid"], 4000, 2, 3, 3, torch.float32,
                                            {1: "atomic", 2: "tiled"}[algo])
    ws = torch.empty(max(ws_n, 256), dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rot_cm = p["rot"].transpose(1, 2).contiguous()
    rc = dpr_amd.lib().dpr_raster_channels_ex_f32(
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), algo, 0, 3, 3,
        g.ctypes.data_as(ctypes.c_void_p), 4000, 2, 3, ptr(out), ptr(p["points"]), ptr(rot_cm), ptr(p["trans"]),
        None, ptr(p["ow"]), None, ptr(ws), ws.numel())
    assert rc == 0, _lib.last_error()
    ref = dpr_amd.raster(p["grid"], p["points"], p["rot"], p["trans"], None, p["ow"], None,
                         algo={1: "atomic", 2: "tiled"}[algo])
    for c in range(3):
        assert_close(plane(out, c, 3), ref, 5e-5, f"plane {c}")
        if algo == _lib.ALGO_TILED:
            assert torch.equal(plane(out, c, 3), ref)
