"""Forward-mode derivative of the smooth splat on the GPU (dpr_raster_smooth_jvp_ex_*, raster_smooth_jvp,
raster_smooth_ad under forward_ad) against the fp64 numpy reference tests/smooth_jvp_reference.py, the adjoint
identity with the library's own pullback, central differences of the library's own forward, and K = 1 calls.

The case is that of tests/test_smooth_gpu.py (grids (37, 19, 21) / (150, 37): three tiles and a partial last tile per
axis; 20 000 points in +-1.15 with an empty slab, 2 000 points in one cell, the corner-cell points), its values
rounded to fp32 once so that one fp64 reference serves both dtypes.  Tolerances, norm-wise: against the reference
1e-10 fp64 / 1e-4 fp32 (tests/test_jvp_gpu.py's; the fp32 numpy reference itself is within 8.5e-6 of fp64 on this
case, worst for points_dot alone on (2,2), where the packed cell cancels); tiled against atomic, linearity
1e-12 / 1e-5; NULL against zero tangents and a K = 16 plane against its K = 1 call 1e-12 / 1e-6.

The fp32 1e-6 bounds are what the ATOMIC path's combine of equal cells within a wave (k_smooth_jvp_atomic) is there
for: the 2 000 packed points add ~1e2-sized deposits of either sign onto the same cells, and with one fp32 global
atomic per (point, cell) in arrival order two identical calls differed by 2.6e-7 .. 1.2e-6 norm-wise on an MI355X.
With one atomic per (wave, cell) they differ by 4e-8 .. 1.5e-7.  The TILED path, which sums in f64 LDS cells, repeats
to 1e-9.  See test_sixteen_tangents_equal_sixteen_single_calls for the figures."""
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import dpr_amd
from tests import smooth_jvp_reference as JR
from tests import smooth_reference as SR
from tests.test_parity_gpu import T, grid_to_dev
from tests.test_smooth_gpu import _case

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
ALGOS = ("atomic", "tiled")
KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
BK = [(1, 1), (3, 2), (1, 5)]  # K != B: a swapped plane index (k * B + b) fails


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def tol(npdt, f64=1e-10, f32=1e-4):
    return f64 if npdt == np.float64 else f32


def assert_close(actual, expected, rtol, what=""):
    a = actual.detach().cpu().double().numpy() if isinstance(actual, torch.Tensor) else np.asarray(actual, float)
    e = expected.detach().cpu().double().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected, float)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    assert np.all(np.isfinite(a)), f"{what}: non-finite values"
    err = np.linalg.norm((a - e).ravel())
    scale = max(np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel()))
    assert err <= rtol * scale + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def primal(n_in, n_out):
    """The case's inputs rounded to fp32 (exact in either dtype); never modified."""
    c = _case(n_in, n_out)
    p = dict(grid=c["grid"], points=_r32(c["points"]), rot=_r32(c["rot"]), trans=_r32(c["trans"]), bg=_r32(c["bg"]),
             ow=_r32(c["ow"]), pw=_r32(c["pw"]), g=_r32(c["g"]))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def tangents(n_in, n_out, B, K, seed=0):
    """All six tangents ~ N(0, 1), rounded to fp32; rotation_dot is not symmetric (a row-major read fails)."""
    rng = np.random.default_rng(1000 * seed + 10 * B + K)
    P = len(primal(n_in, n_out)["points"])
    t = dict(points=rng.normal(size=(K, P, n_in)), rotation=rng.normal(size=(K, B, n_out, n_in)),
             translation=rng.normal(size=(K, B, n_out)), background=rng.normal(size=(K, B)),
             out_weight=rng.normal(size=(K, B)), point_weight=rng.normal(size=(K, P)))
    t = {k: _r32(v) for k, v in t.items()}
    for v in t.values():
        v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference(n_in, n_out, B, K, kinds=KINDS, seed=0):
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K, seed)
    out = JR.raster_smooth_jvp(p["grid"], p["points"], p["rot"][:B], p["trans"][:B], p["ow"][:B], p["pw"], K=K,
                               **{k + "_dot": t[k] for k in kinds})
    out.setflags(write=False)
    return out


def dev_primal(p, dev, npdt, B):
    return [T(p[k][:B].astype(npdt) if k not in ("points", "pw") else p[k].astype(npdt), dev)
            for k in ("points", "rot", "trans", "bg", "ow", "pw")]


def dev_tangents(t, dev, npdt, kinds=KINDS):
    return {k + "_dot": T(t[k].astype(npdt), dev) for k in kinds}


def jvp(p, t, dev, npdt, B, K, algo, kinds=KINDS, **kw):
    return dpr_amd.raster_smooth_jvp(p["grid"], *dev_primal(p, dev, npdt, B), **dev_tangents(t, dev, npdt, kinds),
                                     tangents=K, algo=algo, **kw)


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("kinds", [KINDS] + [(k,) for k in KINDS], ids=lambda k: "all" if len(k) > 1 else k[0])
@pytest.mark.parametrize("B,K", BK)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_matches_the_reference(dev, n_in, n_out, B, K, kinds):
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K)
    ref = reference(n_in, n_out, B, K, kinds)
    assert np.linalg.norm(ref) > 0
    for npdt, tdt in DTYPES:
        for algo in ALGOS:
            out = jvp(p, t, dev, npdt, B, K, algo, kinds)
            assert tuple(out.shape) == p["grid"] + (K, B) and out.dtype == tdt
            assert_close(out, ref, tol(npdt), f"{algo} {npdt.__name__} B={B} K={K} {kinds}")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_equals_atomic_and_auto_is_one_of_them(dev, npdt, tdt, n_in, n_out):
    p, t = primal(n_in, n_out), tangents(n_in, n_out, 3, 2)
    a = jvp(p, t, dev, npdt, 3, 2, "atomic")
    ti = jvp(p, t, dev, npdt, 3, 2, "tiled")
    assert_close(ti, a, tol(npdt, 1e-12, 1e-5), "tiled vs atomic")
    assert dpr_amd.resolve_algo_smooth_jvp(p["grid"], len(p["points"]), 3, n_in, 2) in ALGOS
    assert_close(jvp(p, t, dev, npdt, 3, 2, "auto"), a, tol(npdt, 1e-12, 1e-5), "auto vs atomic")
    # a caller's workspace of the queried size serves the tiled path
    need = dpr_amd.workspace_bytes_smooth_jvp(p["grid"], len(p["points"]), 3, n_in, 2, tdt, algo="tiled")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert_close(jvp(p, t, dev, npdt, 3, 2, "tiled", workspace=ws), a, tol(npdt, 1e-12, 1e-5), "caller's workspace")


@pytest.mark.parametrize("algo", ALGOS)
def test_sixteen_tangents_equal_sixteen_single_calls(dev, algo):
    """fp32, (3,3): plane k of one K = 16 call against the K = 1 call on tangent k, norm-wise within 1e-6.

    Measured on an MI355X, relative differences over the 16 planes.  tiled: 3.5e-10 .. 4.9e-9 (two K = 1 calls differ
    by 2.4e-10 .. 1.2e-9).  atomic: 7.1e-8 .. 3.2e-7 (two identical K = 1 atomic calls: 4.3e-8 .. 1.5e-7): the
    deposits are the same bits, the arrival order of the fp32 global atomics is not.  Before the atomic kernel combined
    the lanes of a wave that share a cell, with one atomic per (point, cell), the same figures were 2.3e-7 .. 1.5e-6
    and 2.6e-7 .. 1.2e-6 -- the cells of the 2 000 packed points take deposits of ~1e2 with either sign -- and this
    test failed in half of the runs.  Both paths are 1.1e-7 .. 8.7e-7 from the fp64 reference."""
    n_in, n_out, B, K, npdt = 3, 3, 1, 16, np.float32
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K)
    out = jvp(p, t, dev, npdt, B, K, algo)
    assert tuple(out.shape) == p["grid"] + (K, B)
    args = dev_primal(p, dev, npdt, B)
    for k in range(K):
        one = {n + "_dot": T(t[n][k].astype(npdt), dev) for n in KINDS}
        single = dpr_amd.raster_smooth_jvp(p["grid"], *args, **one, algo=algo)  # tangents=None: primal shapes
        assert tuple(single.shape) == p["grid"] + (B,)
        assert_close(out[..., k, :], single, 1e-6, f"{algo} plane {k}")


# ------------------------------------------------------------------ 2. tangent handling
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_null_zero_linearity_and_rejected_points(dev, npdt, tdt, n_in, n_out, algo):
    """NULL against zero tangents and NaN tangents of rejected points within 1e-12 / 1e-6, linearity within
    1e-12 / 1e-5.  The fp32 atomic cases of the two 1e-6 comparisons compare two atomic calls whose deposits are the
    same bits: they measure the path's run-to-run noise on this cloud (see the module docstring)."""
    B, K = 3, 2
    p = primal(n_in, n_out)
    v, w = tangents(n_in, n_out, B, K, seed=1), tangents(n_in, n_out, B, K, seed=2)
    # NULL against zero tangents
    some = ("rotation", "point_weight")
    a = jvp(p, v, dev, npdt, B, K, algo, some)
    zeros = {k: (v[k] if k in some else np.zeros_like(v[k])) for k in KINDS}
    assert_close(jvp(p, zeros, dev, npdt, B, K, algo), a, tol(npdt, 1e-12, 1e-6), "NULL vs zero")
    none = dpr_amd.raster_smooth_jvp(p["grid"], *dev_primal(p, dev, npdt, B), tangents=K, algo=algo)
    assert not bool(none.any())
    # J (2 v - 3 w) = 2 J v - 3 J w
    mix = {k: 2 * v[k] - 3 * w[k] for k in KINDS}
    jv, jw = jvp(p, v, dev, npdt, B, K, algo), jvp(p, w, dev, npdt, B, K, algo)
    assert_close(jvp(p, mix, dev, npdt, B, K, algo), 2 * jv.double() - 3 * jw.double(), tol(npdt, 1e-12, 1e-5),
                 "linearity")
    # NaN tangents at points that no pose accepts leave no trace
    rejected = np.ones(len(p["points"]), bool)
    for _b, idx, *_ in SR._terms(p["grid"], p["points"].astype(npdt), p["rot"].astype(npdt), p["trans"].astype(npdt),
                                 npdt):
        rejected[idx] = False
    # (points within 1e-3 cells of the acceptance border could flip between numpy and the device: left alone)
    coord = (np.einsum("bnj,pj->bpn", p["rot"], p["points"]) + p["trans"][:, None, :] + 1) * np.asarray(p["grid"]) / 2
    near = (np.abs(coord + 1) < 1e-3) | (np.abs(coord - (np.asarray(p["grid"]) + 1)) < 1e-3)
    rejected &= ~near.any(axis=(0, 2))
    assert rejected.sum() > 100
    bad = {k: v[k].copy() for k in KINDS}
    bad["points"][:, rejected] = np.nan
    bad["point_weight"][:, rejected] = np.nan
    out = jvp(p, bad, dev, npdt, B, K, algo)
    assert bool(torch.isfinite(out).all())
    assert_close(out, jv, tol(npdt, 1e-12, 1e-6), "NaN tangents of rejected points")


# ------------------------------------------------------------------ 3. small clouds
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_small_clouds(dev, npdt, tdt, n_in, n_out, algo):
    p = primal(n_in, n_out)
    grid, B, K = p["grid"], 3, 2
    t = tangents(n_in, n_out, B, K)
    rot, trans, ow = p["rot"], p["trans"], p["ow"]
    pose_t = {k + "_dot": T(t[k].astype(npdt), dev) for k in ("rotation", "translation", "background", "out_weight")}
    # P = 0: the background tangent alone
    out = dpr_amd.raster_smooth_jvp(grid, torch.zeros((0, n_in), dtype=tdt, device=dev), T(rot.astype(npdt), dev),
                                    T(trans.astype(npdt), dev), None, T(ow.astype(npdt), dev), tangents=K, algo=algo,
                                    **pose_t)
    want = np.broadcast_to(t["background"].astype(npdt), grid + (K, B))
    assert np.array_equal(out.cpu().numpy(), want)
    # one point: in a corner cell; with centre cell -1 and with centre cell n_0 on axis 0 (pose 0 is the identity:
    # the clamped-tile cases of the tiled path)
    n0 = grid[0]
    corner = np.zeros(n_in)
    corner[:n_out] = [1 - 1.0 / n for n in grid]
    below, above = np.full(n_in, 0.21), np.full(n_in, 0.21)
    below[0], above[0] = -1 - 1.0 / n0, 1 + 1.0 / n0
    rng = np.random.default_rng(3)
    for name, x in (("corner", corner), ("centre cell -1", below), ("centre cell n_0", above)):
        pts = _r32(x[None])
        j0 = np.floor((pts[0, 0] + 1) * n0 / 2)
        assert j0 == {"corner": n0 - 1, "centre cell -1": -1, "centre cell n_0": n0}[name]
        pd, pwd = _r32(rng.normal(size=(K, 1, n_in))), _r32(rng.normal(size=(K, 1)))
        ref = JR.raster_smooth_jvp(grid, pts, rot, trans, ow, None, K=K, points_dot=pd, point_weight_dot=pwd,
                                   **{k + "_dot": t[k] for k in ("rotation", "translation", "background",
                                                                 "out_weight")})
        assert np.abs(ref[..., 0] - t["background"][:, 0]).max() > 1e-3  # pose 0 does deposit
        out = dpr_amd.raster_smooth_jvp(grid, T(pts.astype(npdt), dev), T(rot.astype(npdt), dev),
                                        T(trans.astype(npdt), dev), None, T(ow.astype(npdt), dev), tangents=K,
                                        algo=algo, points_dot=T(pd.astype(npdt), dev),
                                        point_weight_dot=T(pwd.astype(npdt), dev), **pose_t)
        assert_close(out, ref, tol(npdt), f"{algo} one point, {name}")


# ------------------------------------------------------------------ 4. derivative identities on the device
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_adjoint_identity_with_the_pullback(dev, npdt, tdt, n_in, n_out):
    B, K = 3, 2
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K)
    g = grid_to_dev(p["g"].astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_(g, *dev_primal(p, dev, npdt, B))
    grads = [x.double().cpu().numpy() for x in pb]
    for algo in ALGOS:
        jv = jvp(p, t, dev, npdt, B, K, algo).double().cpu().numpy()
        for k in range(K):
            lhs = float((jv[..., k, :] * p["g"]).sum())
            rhs = sum(float((t[name][k] * grad).sum()) for name, grad in zip(KINDS, grads))
            bound = tol(npdt, 1e-11, 1e-4) * np.linalg.norm(jv[..., k, :]) * np.linalg.norm(p["g"])
            print(f"({n_in},{n_out}) {npdt.__name__} {algo} k={k}: |lhs - rhs| = {abs(lhs - rhs):.3e}, "
                  f"bound {bound:.3e}")
            assert abs(lhs - rhs) <= bound, (algo, k, lhs, rhs)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences_of_the_forward(dev, n_in, n_out):
    """fp64: differences of raster_smooth along the joint tangent with step 1e-7, norm-wise within 1e-6."""
    B, K, npdt = 3, 2, np.float64
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K)
    h = 1e-7
    names = ("points", "rot", "trans", "bg", "ow", "pw")
    base = [p[k] if k in ("points", "pw") else p[k][:B] for k in names]
    for algo in ALGOS:
        jv = jvp(p, t, dev, npdt, B, K, algo)
        for k in range(K):
            f = lambda sign: dpr_amd.raster_smooth(
                p["grid"], *[T(x + sign * h * t[kind][k], dev) for x, kind in zip(base, KINDS)]).double()
            fd = (f(+1) - f(-1)) / (2 * h)
            assert_close(jv[..., k, :], fd, 1e-6, f"{algo} k={k}")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_out_dot_is_continuous_across_a_cell_face(dev, n_in, n_out, algo):
    """One point moved from 1e-9 cells below to 1e-9 above a cell face (fp64, identity pose): out_dot for a points_dot
    tangent agrees within 1e-6 -- the continuity the N-linear JVP does not have."""
    grid = primal(n_in, n_out)["grid"]
    n0 = grid[0]
    rot, trans = T(np.eye(n_out, n_in), dev), T(np.zeros(n_out), dev)
    pd = T(np.array([[0.7, -1.3, 0.4][:n_in]]), dev)
    outs = []
    for eps in (-1e-9, 1e-9):
        x = np.full((1, n_in), 0.21)
        x[0, 0] = -1 + 2.0 * (20 + eps) / n0  # coord_0 = 20 -+ 1e-9
        assert np.floor((x[0, 0] + 1) * n0 / 2) == (19 if eps < 0 else 20)
        outs.append(dpr_amd.raster_smooth_jvp(grid, T(x, dev), rot, trans, points_dot=pd, algo=algo))
    assert float(outs[0].abs().max()) > 0
    assert_close(outs[0], outs[1], 1e-6, "either side of the face")


# ------------------------------------------------------------------ 5. raster_smooth_ad in forward mode
@pytest.mark.parametrize("algo", ["auto", "atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_forward_mode_through_autograd(dev, npdt, tdt, algo):
    """raster_smooth_ad under forward_ad.dual_level: raises without a jvp on the autograd function."""
    n_in, n_out, B = 3, 3, 3
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, 1)
    args = dev_primal(p, dev, npdt, B)
    tans = [T(t[k][0].astype(npdt), dev) for k in KINDS]
    want = dpr_amd.raster_smooth_jvp(p["grid"], *args, **{k + "_dot": v for k, v in zip(KINDS, tans)}, algo=algo)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(a, v) for a, v in zip(args, tans)]
        out = dpr_amd.raster_smooth_ad(p["grid"], *duals, algo=algo)
        primal_out, tangent = fwAD.unpack_dual(out)
    assert tangent is not None and tangent.shape == want.shape
    assert_close(tangent, want, tol(npdt, 1e-12, 1e-5), f"forward mode, {algo}")
    assert_close(primal_out, dpr_amd.raster_smooth(p["grid"], *args, algo=algo), tol(npdt, 1e-12, 1e-5), "primal")
    # a single pose; only the rotation carries a tangent, the optional arguments are constants
    R, tr, Rd = args[1][1], args[2][1], tans[1][1]
    with fwAD.dual_level():
        out = dpr_amd.raster_smooth_ad(p["grid"], args[0], fwAD.make_dual(R, Rd), tr, None, 2.0, algo=algo)
        tangent = fwAD.unpack_dual(out).tangent
    want = dpr_amd.raster_smooth_jvp(p["grid"], args[0], R, tr, None, 2.0, rotation_dot=Rd, algo=algo)
    assert tangent.shape == p["grid"]
    assert_close(tangent, want, tol(npdt, 1e-12, 1e-5), f"rotation tangent alone, {algo}")


def test_forward_mode_and_reverse_mode_jacobians_agree(dev):
    """6 points on a (6, 5) grid, fp64: the Jacobian of raster_smooth_ad from torch.autograd.functional.jacobian
    (reverse mode) against the one assembled column by column from dual tensors (its forward-mode strategy needs a
    vmap rule, which a function that calls into the library has not)."""
    rng = np.random.default_rng(21)
    grid, P, n_in, n_out = (6, 5), 6, 2, 2
    vals = [rng.uniform(-1.1, 1.1, size=(P, n_in)), np.linalg.qr(rng.normal(size=(2, 2)))[0], rng.normal(size=2) * 0.05,
            rng.normal(size=()), rng.uniform(0.5, 1.5, size=()), rng.uniform(0.5, 1.5, size=P)]
    args = [torch.tensor(v, dtype=torch.float64, device=dev) for v in vals]
    f = lambda *xs: dpr_amd.raster_smooth_ad(grid, *xs, algo="atomic")
    J = torch.autograd.functional.jacobian(f, tuple(args))
    cells = int(np.prod(grid))
    for i, (a, Ji) in enumerate(zip(args, J)):
        Ji = Ji.reshape(cells, -1)
        assert float(Ji.abs().max()) > 0
        for col in range(a.numel()):
            e = torch.zeros(a.numel(), dtype=torch.float64, device=dev)
            e[col] = 1
            with fwAD.dual_level():
                xs = list(args)
                xs[i] = fwAD.make_dual(a, e.reshape(a.shape))
                tangent = fwAD.unpack_dual(f(*xs)).tangent
            err = float((tangent.reshape(-1) - Ji[:, col]).abs().max())
            assert err <= 1e-12 * max(1.0, float(Ji.abs().max())), (KINDS[i], col, err)


# ------------------------------------------------------------------ 6. refused calls leave out_dot untouched
def test_refused_calls_leave_out_dot_untouched(dev):
    n_in, n_out, B, K, npdt = 3, 3, 3, 2, np.float32
    p, t = primal(n_in, n_out), tangents(n_in, n_out, B, K)
    args, kw = dev_primal(p, dev, npdt, B), dev_tangents(t, dev, npdt)
    out = dpr_amd.empty_channel_grid(p["grid"], K, B, torch.float32, dev)
    out.fill_(7.0)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_smooth_jvp_(out, *args, **kw, tangents=K, algo="chunked")
    with pytest.raises(ValueError):  # a workspace shorter than the queried size
        short = torch.empty(dpr_amd.workspace_bytes_smooth_jvp(p["grid"], len(p["points"]), B, n_in, K, algo="tiled")
                            - 256, dtype=torch.uint8, device=dev)
        dpr_amd.raster_smooth_jvp_(out, *args, **kw, tangents=K, algo="tiled", workspace=short)
    with pytest.raises(dpr_amd.DprError):  # K = 17
        dpr_amd.raster_smooth_jvp_(out, *args, **kw, tangents=17)
    with pytest.raises(dpr_amd.DimensionMismatch):  # the pair (2, 3)
        dpr_amd.raster_smooth_jvp_(out, args[0][:, :2].contiguous(), torch.zeros(B, 3, 2, device=dev),
                                   torch.zeros(B, 3, device=dev), tangents=K)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the same four through the C entry point, which reports a status and launches nothing
    import ctypes

    from dpr_amd import _lib
    L = _lib.lib()
    grid = np.asarray(p["grid"], dtype=np.int64)
    gp = grid.ctypes.data_as(ctypes.c_void_p)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    pts, rot, trans, _bg, ow, pw = args
    rot_cm = rot.transpose(1, 2).contiguous()
    need = L.dpr_workspace_bytes_smooth_jvp_ex_f32(_lib.ALGO_TILED, 0, n_in, n_out, gp, len(pts), B, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(algo=_lib.ALGO_ATOMIC, ni=n_in, no=n_out, k=K, wsb=0):
        return L.dpr_raster_smooth_jvp_ex_f32(st, algo, 0, ni, no, gp, len(pts), B, k, ptr(out), ptr(pts), ptr(rot_cm),
                                              ptr(trans), ptr(ow), ptr(pw), ptr(kw["points_dot"]), None, None, None,
                                              None, None, ptr(ws) if wsb else None, wsb)

    assert call(k=17) == _lib.ERR_INVALID_ARG
    assert call(ni=2, no=3) == _lib.ERR_UNSUPPORTED_DIMS
    assert call(algo=_lib.ALGO_CHUNKED) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(algo=_lib.ALGO_TILED, wsb=need - 256) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(algo=_lib.ALGO_TILED, wsb=need) == _lib.OK
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
