"""Point sampling on the GPU (dpr_sample_ex_*, dpr_sample_pullback_ex_*).

The ground truth is the oracle's pullback: values[:, b] is the ds_dpoint_weight of `raster_pullback` with
ds_dout = image_b and out_weight 1; the sampling pullback is per-pose `raster` (ds_dimage) and per-pose
`raster_pullback` with point_weight = ds_dvalues[:, b] (the geometric gradients).  Tolerances are those of
tests/test_parity_gpu.py."""
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
PAIRS = [(2, 2), (3, 3), (3, 2), (2, 3), (1, 2), (4, 4)]


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


def problem(dev, tdt, n_in, n_out, B, P=3000, grid_n=16, seed=0):
    """Single pose (B = None) or a batch; image and ds_dvalues random normal."""
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B or 1, grid_n=grid_n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    image = rng.normal(size=d.grid + (B or 1,))
    dv = rng.normal(size=(P, B or 1))
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    img = dpr_amd.to_grid_layout(to(image))
    p = dict(points=to(d.points), grid=d.grid, image_np=image, dv_np=dv, B=B)
    if B is None:
        p.update(rot=to(d.rotations[0]), trans=to(d.translations[0]), image=img[..., 0], dv=to(dv[:, 0]))
    else:
        p.update(rot=to(d.rotations), trans=to(d.translations), image=img, dv=to(dv))
    return p


def np_pose(p, b):
    R = p["rot"].double().cpu().numpy()
    t = p["trans"].double().cpu().numpy()
    if R.ndim == 2:
        R, t = R[None], t[None]
    return R[b:b + 1], t[b:b + 1]


def oracle_values(p, b, npdt):
    R, t = np_pose(p, b)
    pts = p["points"].double().cpu().numpy()
    img = p["image"].double().cpu().numpy()
    img_b = img[..., None] if p["B"] is None else img[..., b:b + 1]
    return oracle.raster_pullback(img_b, pts, R, t, out_weight=np.ones(1), dtype=npdt).point_weight


def column(v, b, single):
    return v if single else v[:, b]


# ------------------------------------------------------------------ 1. forward against the oracle
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [None, 1, 3])
def test_forward_matches_the_oracle_pullback(dev, n_in, n_out, npdt, tdt, B):
    p = problem(dev, tdt, n_in, n_out, B, grid_n=8 if n_out == 4 else 16)
    v = dpr_amd.sample(p["image"], p["points"], p["rot"], p["trans"])
    torch.cuda.synchronize()
    P = p["points"].shape[0]
    assert v.shape == ((P,) if B is None else (P, B)) and v.dtype == tdt
    if B is not None:
        assert v.t().is_contiguous()  # point index fastest
    for b in range(B or 1):
        assert_close(column(v, b, B is None), oracle_values(p, b, npdt), tol(npdt, "out"), f"values[:, {b}]")
    if B == 1:
        # the same helper in the same order as the device's own direct pullback: bit-identical
        pb = dpr_amd.raster_pullback_(p["image"], p["points"], p["rot"], p["trans"], None,
                                      torch.ones(1, dtype=tdt, device=dev), torch.ones(P, dtype=tdt, device=dev),
                                      algo="atomic")
        assert torch.equal(v[:, 0], pb.point_weight)


# ------------------------------------------------------------------ 2. pullback against per-pose oracle calls
PB_CASES = [("atomic", i, o) for (i, o) in PAIRS] + [("tiled", i, o) for (i, o) in ((2, 2), (3, 3), (3, 2))] + \
    [("auto", 3, 3)]


def _rounding_level(got, ref, what):
    """fp32 tiled planes of weights that span more than the fixed-point range guard (2^10, dpr_device.h): the
    tiled forward sums them with f64 atomics, whose order varies run to run (include/dpr.h, SUMMATION ORDER), so
    the plane can differ from another call with the same weights at fp32 rounding level."""
    d = (got.double() - ref.double()).abs().max().item()
    assert d <= 4e-6 * ref.double().abs().max().item(), f"{what}: {d}"


@pytest.mark.parametrize("algo,n_in,n_out", PB_CASES)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [None, 3])
def test_pullback_matches_per_pose_oracle_calls(dev, algo, n_in, n_out, npdt, tdt, B):
    p = problem(dev, tdt, n_in, n_out, B, grid_n=8 if n_out == 4 else 16, seed=1)
    pb = dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], algo=algo)
    torch.cuda.synchronize()
    pts = p["points"].double().cpu().numpy()
    img = p["image"].double().cpu().numpy()
    dv = p["dv"].double().cpu().numpy().reshape(pts.shape[0], -1)
    single = B is None
    sum_pts = np.zeros_like(pts)
    for b in range(B or 1):
        R, t = np_pose(p, b)
        ref_img = oracle.raster(p["grid"], pts, R, t, None, None, dv[:, b], dtype=npdt)[..., 0]
        got_img = pb.image if single else pb.image[..., b]
        assert_close(got_img, ref_img, tol(npdt, "out"), f"ds_dimage[.., {b}]")
        img_b = img[..., None] if single else img[..., b:b + 1]
        r = oracle.raster_pullback(img_b, pts, R, t, np.ones(1), dv[:, b], dtype=npdt)
        assert_close(pb.rotation if single else pb.rotation[b], r.rotation[0], tol(npdt, "pose"), f"ds_drotation[{b}]")
        assert_close(pb.translation if single else pb.translation[b], r.translation[0], tol(npdt, "pose"),
                     f"ds_dtranslation[{b}]")
        sum_pts += r.points
        if algo == "tiled" and tdt == torch.float32:
            args = (p["grid"], p["points"], p["rot"] if single else p["rot"][b],
                    p["trans"] if single else p["trans"][b])
            w = p["dv"] if single else p["dv"][:, b].contiguous()
            ref = dpr_amd.raster(*args, point_weight=w, algo="tiled")
            _rounding_level(got_img, ref, f"ds_dimage plane {b}")
    assert_close(pb.points, sum_pts, tol(npdt, "points"), "ds_dpoints")


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
@pytest.mark.parametrize("B", [None, 3])
def test_tiled_fp32_planes_match_the_tiled_forward(dev, n_in, n_out, B):
    """ds_dvalues whose magnitudes stay inside the fixed-point range guard (here within 4x).  Each plane of the
    fp32 TILED pullback is computed by dpr_raster_ex_f32(DPR_ALGO_TILED) with point_weight = ds_dvalues[:, b]:
      * 3-D: that forward sums exactly in fixed point and reproduces itself bit for bit, so the plane must be
        BIT-IDENTICAL to it -- no tolerance, no escape;
      * 2-D: at this size that forward does not reproduce itself (two identical calls differ by 1 ulp in a few
        dozen of the 256 cells), so the plane is held to the same fp32 rounding level."""
    p = problem(dev, torch.float32, n_in, n_out, B, seed=2)
    rng = np.random.default_rng(12)
    P = p["points"].shape[0]
    w = rng.choice([-1.0, 1.0], size=(P, B or 1)) * rng.uniform(0.25, 1.0, size=(P, B or 1))
    dv = torch.as_tensor(w, dtype=torch.float32, device=dev)
    dv = dv[:, 0].contiguous() if B is None else dv
    pb = dpr_amd.sample_pullback_(dv, p["image"], p["points"], p["rot"], p["trans"], algo="tiled")
    for b in range(B or 1):
        args = (p["grid"], p["points"], p["rot"] if B is None else p["rot"][b],
                p["trans"] if B is None else p["trans"][b])
        ref = dpr_amd.raster(*args, point_weight=dv if B is None else dv[:, b].contiguous(), algo="tiled")
        got = pb.image if B is None else pb.image[..., b]
        if n_out == 3:
            assert torch.equal(got, ref), f"plane {b}: not bit-identical to the tiled forward"
        else:
            _rounding_level(got, ref, f"plane {b}")


# ------------------------------------------------------------------ 3. adjoint identity between two GPU operators
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2), (2, 3)])
def test_adjoint_identity(dev, n_in, n_out):
    rng = np.random.default_rng(3)
    B, P = 3, 5000
    p = problem(dev, torch.float64, n_in, n_out, B, P=P, seed=3)
    pw = torch.as_tensor(rng.uniform(-1, 1, size=P), device=dev)
    bg = torch.as_tensor(rng.normal(size=B), device=dev)
    ow = torch.as_tensor(rng.uniform(0.5, 2, size=B), device=dev)
    out = dpr_amd.raster(p["grid"], p["points"], p["rot"], p["trans"], bg, ow, pw)
    v = dpr_amd.sample(p["image"], p["points"], p["rot"], p["trans"])
    lhs = ((out - bg) * p["image"]).reshape(-1, B).sum(0)
    rhs = ow * (pw[:, None] * v).sum(0)
    err = (lhs - rhs).abs().max().item()
    assert err <= 1e-12 * max(lhs.abs().max().item(), 1.0), (lhs, rhs)


# ------------------------------------------------------------------ 4. gradcheck
def _points_off_boundaries(rng, P, n_in, R, t, grid, margin=0.05):
    """Points whose cell coordinates keep `margin` from every cell boundary under every pose (the interpolant
    is only piecewise smooth)."""
    keep = []
    while len(keep) < P:
        x = 0.4 * rng.normal(size=n_in)
        c = (np.einsum("bij,j->bi", R, x) + t + 1) * (np.asarray(grid) / 2) - 0.5
        f = c - np.floor(c)
        if np.all((f > margin) & (f < 1 - margin)) and np.all((c > 0) & (c < np.asarray(grid) - 1)):
            keep.append(x)
    return np.stack(keep)


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3)])
def test_gradcheck_sample_ad(dev, n_in, n_out):
    rng = np.random.default_rng(4)
    B, grid = 2, (6,) * n_out
    R = D.random_rotations(rng, B, n_in)[:, :n_out, :]
    t = 0.05 * rng.normal(size=(B, n_out))
    pts = _points_off_boundaries(rng, 12, n_in, R, t, grid)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev).requires_grad_()
    image = to(rng.normal(size=grid + (B,)))
    args = (image, to(pts), to(R), to(t))
    assert torch.autograd.gradcheck(lambda *a: dpr_amd.sample_ad(*a), args, eps=1e-6, atol=1e-6, rtol=1e-5,
                                    nondet_tol=1e-12)


# ------------------------------------------------------------------ 5. edge cases
def test_rejected_points_give_zero_and_no_gradient(dev):
    n = 8
    eye, zero = torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(6)
    inside = 0.3 * rng.normal(size=(50, 3))
    bad = np.array([[5.0, 0, 0], [-1.125, 0, 0], [0, 1.13, 0], [np.nan, 0, 0], [0, 0, np.inf]])
    pts = torch.as_tensor(np.concatenate([inside, bad]), device=dev)
    img = dpr_amd.to_grid_layout(torch.as_tensor(rng.normal(size=(n, n, n)), device=dev))
    v = dpr_amd.sample(img, pts, eye, zero)
    assert torch.all(v[50:] == 0)
    dv = torch.as_tensor(rng.normal(size=55), device=dev)
    pb = dpr_amd.sample_pullback_(dv, img, pts, eye, zero, algo="atomic")
    pb_in = dpr_amd.sample_pullback_(dv[:50].contiguous(), img, pts[:50].contiguous(), eye, zero, algo="atomic")
    assert torch.all(pb.points[50:] == 0)
    assert_close(pb.image, pb_in.image, 1e-12, "ds_dimage without the rejected points")
    assert_close(pb.rotation, pb_in.rotation, 1e-12, "ds_drotation")
    assert_close(pb.translation, pb_in.translation, 1e-12, "ds_dtranslation")
    assert torch.isfinite(pb.image).all() and torch.isfinite(pb.rotation).all()


def test_null_outputs_are_skipped_and_values_written_in_place(dev):
    p = problem(dev, torch.float64, 3, 3, 3, seed=7)
    full = dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], algo="atomic")
    for need in (("image",), ("points",), ("rotation", "translation"), ("points", "image")):
        part = dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], need=need,
                                        algo="atomic")
        for name in dpr_amd.SamplePullbackResult._fields:
            if name in need:
                assert_close(getattr(part, name), getattr(full, name), 1e-12, f"{need}: {name}")
            else:
                assert getattr(part, name) is None
    # ds_dimage alone on the tiled path: no image read at all (the geometric kernel is skipped)
    part = dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], need=("image",),
                                    algo="tiled")
    assert_close(part.image, full.image, 1e-10, "tiled ds_dimage alone")
    # caller buffers are overwritten and returned by identity
    buf = torch.full((3, p["points"].shape[0]), 7.0, dtype=torch.float64, device=dev).t()
    out = dpr_amd.sample_(buf, p["image"], p["points"], p["rot"], p["trans"])
    assert out is buf
    assert_close(buf, dpr_amd.sample(p["image"], p["points"], p["rot"], p["trans"]), 0, "in place")
    d_pts = torch.full_like(full.points, 3.0)
    r = dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], ds_dpoints=d_pts,
                                 need=("points",))
    assert r.points is d_pts
    assert_close(d_pts, full.points, 1e-12, "ds_dpoints in place")


# ------------------------------------------------------------------ 6. bad arguments on the device
def test_errors_leave_outputs_untouched(dev):
    p = problem(dev, torch.float32, 3, 3, 2, seed=8)
    P = p["points"].shape[0]
    sentinel = torch.full((2, P), 7.0, device=dev).t()
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.sample_(sentinel, p["image"], p["points"], p["rot"], p["trans"], algo="tiled")
    assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.sample_(sentinel, p["image"][..., :1], p["points"], p["rot"], p["trans"])
    with pytest.raises(ValueError):
        dpr_amd.sample_(torch.full((P, 2), 7.0, device=dev), p["image"], p["points"], p["rot"], p["trans"])
    with pytest.raises(dpr_amd.DprError) as e:
        dpr_amd.sample_pullback_(p["dv"], p["image"], p["points"], p["rot"], p["trans"], algo="chunked")
    assert e.value.code == _lib.ERR_UNSUPPORTED_ALGO
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)
    # C level, real device buffers: a workspace too small for the tiled pullback, a misaligned output
    g = np.asarray(p["grid"], dtype=np.int64)
    gp = g.ctypes.data_as(ctypes.c_void_p)
    img_out = torch.full((2,) + tuple(p["grid"]), 5.0, device=dev)
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=dev)
    fn = _lib.lib().dpr_sample_pullback_ex_f32
    dvc = p["dv"].t().contiguous()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = fn(None, _lib.ALGO_TILED, 0, 3, 3, gp, P, 2, ptr(dvc), ptr(p["image"]), ptr(p["points"]),
            ptr(p["rot"].transpose(1, 2).contiguous()), ptr(p["trans"]), ptr(img_out), None, None, None,
            ptr(ws), ws.numel())
    assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    rc = fn(None, _lib.ALGO_ATOMIC, 0, 3, 3, gp, P, 2, ptr(dvc), ptr(p["image"]), ptr(p["points"]),
            ptr(p["rot"].transpose(1, 2).contiguous()), ptr(p["trans"]), ctypes.c_void_p(img_out.data_ptr() + 2),
            None, None, None, None, 0)
    assert rc == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(img_out == 5.0)


# ------------------------------------------------------------------ 7. full size
def test_full_size_10m_points_256_cubed(dev):
    rng = np.random.default_rng(9)
    P, grid = 10_000_000, (256, 256, 256)
    pts = torch.as_tensor(0.4 * rng.normal(size=(P, 3)), dtype=torch.float32, device=dev)
    R = torch.as_tensor(D.random_rotations(rng, 1)[0], dtype=torch.float32, device=dev)
    t = torch.as_tensor(0.05 * rng.normal(size=3), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(9)
    img = torch.randn(grid[::-1], generator=gen, device=dev).permute(2, 1, 0)
    dv = torch.randn(P, generator=gen, device=dev)
    v = dpr_amd.sample(img, pts, R, t)
    assert dpr_amd.resolve_algo_sample("pullback", grid, P, 1, 3) == "tiled"
    pb = dpr_amd.sample_pullback_(dv, img, pts, R, t)
    torch.cuda.synchronize()
    sub = torch.as_tensor(rng.choice(P, 50_000, replace=False), device=dev)
    spts = pts[sub].double().cpu().numpy()
    Rn, tn = R.double().cpu().numpy()[None], t.double().cpu().numpy()[None]
    imgn = img.double().cpu().numpy()[..., None]
    dvs = dv[sub].double().cpu().numpy()
    r = oracle.raster_pullback(imgn, spts, Rn, tn, np.ones(1), dvs, dtype=np.float32, threaded=True)
    assert_close(v[sub], oracle.raster_pullback(imgn, spts, Rn, tn, np.ones(1), dtype=np.float32,
                                                threaded=True).point_weight, tol(np.float32, "out"), "values")
    assert_close(pb.points[sub], r.points, tol(np.float32, "points"), "ds_dpoints (subsample)")
    # the per-pose sums and ds_dimage over the whole cloud
    full = oracle.raster_pullback(imgn, pts.double().cpu().numpy(), Rn, tn, np.ones(1), dv.double().cpu().numpy(),
                                  dtype=np.float32, threaded=True)
    assert_close(pb.rotation, full.rotation[0], tol(np.float32, "pose"), "ds_drotation")
    assert_close(pb.translation, full.translation[0], tol(np.float32, "pose"), "ds_dtranslation")
    ref_img = oracle.raster(grid, pts.double().cpu().numpy(), Rn, tn, None, None, dv.double().cpu().numpy(),
                            dtype=np.float32, threaded=True)[..., 0]
    assert_close(pb.image, ref_img, tol(np.float32, "out"), "ds_dimage")
