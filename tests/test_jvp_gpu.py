"""Forward-mode derivative of raster on the GPU (dpr_raster_jvp_ex_*, raster_jvp, raster_ad under forward_ad).

Ground truth: the numpy restatement of the definition in tests/test_jvp_abi.py (itself pinned against the
oracle's Jacobian), the adjoint identity with the library's own pullback, and K = 1 calls."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import dpr_amd
from tests import data as D
from tests.test_jvp_abi import KINDS, jvp_reference, random_tangents

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
TILED_PAIRS = [(2, 2), (3, 3), (3, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def tol(npdt):
    return 1e-10 if npdt == np.float64 else 1e-4


def assert_close(actual, expected, rtol, what=""):
    a = actual.detach().cpu().double().numpy() if isinstance(actual, torch.Tensor) else np.asarray(actual)
    e = expected.detach().cpu().double().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    assert np.all(np.isfinite(a)), f"{what}: non-finite values"
    err = np.linalg.norm((a - e).ravel())
    scale = max(np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel()))
    assert err <= rtol * scale + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


class Problem:
    """Primal and K tangents on the host (fp64 values rounded to the test dtype) and on the device."""

    def __init__(self, dev, npdt, tdt, n_in, n_out, B, K, kinds=KINDS, P=2000, grid_n=None, seed=0,
                 weights=True):
        grid_n = grid_n or (8 if n_out == 4 else 16)
        d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B or 1, grid_n=grid_n, seed=seed)
        rng = np.random.default_rng(seed + 17)
        r = lambda a: np.asarray(a, dtype=npdt).astype(np.float64)
        self.grid, self.B, self.K, self.single = d.grid, B or 1, K, B is None
        self.points, self.rot, self.trans = r(d.points), r(d.rotations), r(d.translations)
        self.bg = r(d.backgrounds)
        self.ow = r(rng.uniform(0.5, 2.0, size=self.B)) if weights else None
        self.pw = r(rng.uniform(0.5, 2.0, size=P)) if weights else None
        self.tan = {k: r(v) for k, v in random_tangents(rng, K, P, self.B, n_in, n_out, kinds).items()}
        self.dev, self.tdt, self.npdt = dev, tdt, npdt

    def t(self, a):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=self.dev).to(self.tdt)

    def primal(self):
        s = self.single
        return (self.t(self.points), self.t(self.rot[0] if s else self.rot), self.t(self.trans[0] if s else
                                                                                   self.trans),
                self.t(self.bg[:1] if s else self.bg), self.t(self.ow[:1] if s and self.ow is not None else self.ow),
                self.t(self.pw))

    def tangent_kwargs(self, k=None, zero=()):
        """keyword tangents: all K (leading axis) or only tangent k (primal shapes)"""
        out = {}
        for kind in KINDS:
            v = self.tan.get(kind)
            if v is None:
                if kind not in zero:
                    continue
                v = np.zeros_like(random_tangents(np.random.default_rng(0), self.K, len(self.points), self.B,
                                                  self.points.shape[1], self.rot.shape[1], (kind,))[kind])
            if k is not None:
                v = v[k]
                if self.single and kind in ("rotation", "translation", "background", "out_weight"):
                    v = v[0]
            elif self.single and kind in ("rotation", "translation", "background", "out_weight"):
                v = v[:, 0]
            out[kind + "_dot"] = self.t(v)
        return out

    def jvp(self, algo, k=None, **kw):
        args = self.primal()
        tk = {} if k is not None else dict(tangents=self.K)
        return dpr_amd.raster_jvp(self.grid, *args, **self.tangent_kwargs(k), algo=algo, **tk, **kw)

    def reference(self):
        return jvp_reference(self.grid, self.points, self.rot, self.trans, self.ow, self.pw, self.tan, self.K,
                             cell_dtype=self.npdt)

    def as_kb(self, out):
        """device out_dot of a K-tangent call -> (grid..., K, B) on the host"""
        a = out.detach().cpu().double().numpy()
        return a[..., None] if self.single else a


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,n_in,n_out", [("atomic", i, o) for i, o in PAIRS] +
                         [("tiled", i, o) for i, o in TILED_PAIRS])
def test_jvp_matches_the_restatement(dev, npdt, tdt, algo, n_in, n_out):
    for B in (None, 3):
        cases = [(1, KINDS), (16, KINDS)] + [(5, (k,)) for k in KINDS]
        for K, kinds in cases:
            pr = Problem(dev, npdt, tdt, n_in, n_out, B, K, kinds, seed=K + 7 * n_in + n_out)
            out = pr.jvp(algo)
            assert tuple(out.shape) == tuple(pr.grid) + (K,) + (() if B is None else (B,))
            assert_close(pr.as_kb(out), pr.reference(), tol(npdt), f"{algo} B={B} K={K} {kinds}")


# ------------------------------------------------------------------ 2. adjoint identity with the pullback
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,algos", [(3, 3, ("atomic", "tiled")), (2, 2, ("atomic", "tiled")),
                                              (3, 2, ("atomic", "tiled", "chunked")), (2, 3, ("atomic",))])
def test_adjoint_identity_with_the_pullback(dev, npdt, tdt, n_in, n_out, algos):
    pr = Problem(dev, npdt, tdt, n_in, n_out, 3, 4, P=5000, grid_n=32)
    pts, rot, trans, bg, ow, pw = pr.primal()
    u = dpr_amd.to_grid_layout(torch.randn(tuple(pr.grid) + (3,), dtype=tdt, device=dev))
    for jalgo in ("atomic", "tiled") if (n_in, n_out) in TILED_PAIRS else ("atomic",):
        out = pr.jvp(jalgo)
        for palgo in algos:
            g = dpr_amd.raster_pullback_(u, pts, rot, trans, bg, ow, pw, algo=palgo)
            grads = dict(points=g.points, rotation=g.rotation, translation=g.translation, background=g.background,
                         out_weight=g.out_weight, point_weight=g.point_weight)
            for k in range(pr.K):
                lhs = float((out[..., k, :].double() * u.double()).sum())
                rhs = sum(float((torch.as_tensor(pr.tan[kind][k], device=dev) * grads[kind].double()).sum())
                          for kind in KINDS)
                scale = float(out[..., k, :].double().norm() * u.double().norm())
                assert abs(lhs - rhs) <= (1e-11 if npdt == np.float64 else 1e-4) * scale, (jalgo, palgo, k, lhs,
                                                                                          rhs)


# ------------------------------------------------------------------ 3. K tangents against K = 1 calls
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,n_in,n_out", [("tiled", 3, 3), ("tiled", 2, 2), ("tiled", 3, 2), ("atomic", 3, 3),
                                             ("atomic", 2, 3)])
def test_planes_equal_single_tangent_calls(dev, npdt, tdt, algo, n_in, n_out):
    pr = Problem(dev, npdt, tdt, n_in, n_out, 2, 5, P=4000, grid_n=24)
    out = pr.jvp(algo)
    exact = algo == "tiled" and n_out == 3 and npdt == np.float32
    for k in range(pr.K):
        one = pr.jvp(algo, k=k)
        if exact:
            assert torch.equal(out[..., k, :], one), k
        else:
            assert_close(out[..., k, :], one, 1e-12 if npdt == np.float64 else 1e-6, f"plane {k}")
    if exact:
        assert torch.equal(pr.jvp(algo), out), "fp32 TILED 3-D must be bit-reproducible"


# ------------------------------------------------------------------ 4. TILED against ATOMIC, the range guard
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", TILED_PAIRS)
def test_tiled_agrees_with_atomic_and_the_guard(dev, npdt, tdt, n_in, n_out):
    # (Norm-wise only: the light half of the guard input carries 1e-6 of the norm, so this would pass with every
    # light deposit dropped.  The per-cell check of the guard and the scale, relative to the bounds that reach a
    # cell, is tests/test_families_precision_gpu.py.)
    pr = Problem(dev, npdt, tdt, n_in, n_out, 2, 3, P=6000, grid_n=48)
    assert_close(pr.jvp("tiled"), pr.jvp("atomic"), 1e-12 if npdt == np.float64 else 1e-5, "tiled vs atomic")
    # point_weight tangents spanning 2^20: every (pose, tangent) scope trips the 2^10 guard (f64 LDS atomics)
    g = Problem(dev, npdt, tdt, n_in, n_out, 2, 2, kinds=("point_weight",), P=6000, grid_n=48, seed=3)
    scale = np.where(np.arange(6000) % 2 == 0, 1e-6, 1.0)
    g.tan["point_weight"] = np.asarray(g.tan["point_weight"] * scale, dtype=npdt).astype(np.float64)
    out = g.jvp("tiled")
    assert_close(g.as_kb(out), g.reference(), tol(npdt), "guard tripped")
    assert_close(out, g.jvp("atomic"), 1e-12 if npdt == np.float64 else 1e-5, "guard tripped vs atomic")


# ------------------------------------------------------------------ 5. NULL tangents, linearity, rejected points
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,n_in,n_out", [("tiled", 3, 3), ("atomic", 3, 3), ("atomic", 1, 2)])
def test_null_tangents_linearity_and_rejected_points(dev, npdt, tdt, algo, n_in, n_out):
    exact = algo == "tiled" and npdt == np.float32
    pr = Problem(dev, npdt, tdt, n_in, n_out, 2, 2, kinds=("points", "rotation"), P=3000, grid_n=20)
    args = pr.primal()
    a = pr.jvp(algo)
    b = dpr_amd.raster_jvp(pr.grid, *args, **pr.tangent_kwargs(zero=KINDS), tangents=2, algo=algo)
    if exact:
        assert torch.equal(a, b)
    else:
        assert_close(a, b, 1e-12 if npdt == np.float64 else 1e-6, "NULL vs zero")
    z = dpr_amd.raster_jvp(pr.grid, *args, tangents=3, algo=algo)
    assert torch.count_nonzero(z) == 0
    bgd = torch.tensor([[1.5, -2.0], [0.0, 3.0]], dtype=tdt, device=dev)
    zb = dpr_amd.raster_jvp(pr.grid, *args, background_dot=bgd, tangents=2, algo=algo)
    for k in range(2):
        for bb in range(2):
            assert torch.all(zb[..., k, bb] == bgd[k, bb])
    # linearity: J (2 v - 3 w) = 2 J v - 3 J w
    kw = pr.tangent_kwargs()
    v = {n: t[0] for n, t in kw.items()}
    w = {n: t[1] for n, t in kw.items()}
    comb = {n: 2 * v[n] - 3 * w[n] for n in kw}
    jv = dpr_amd.raster_jvp(pr.grid, *args, **v, algo=algo)
    jw = dpr_amd.raster_jvp(pr.grid, *args, **w, algo=algo)
    jc = dpr_amd.raster_jvp(pr.grid, *args, **comb, algo=algo)
    assert_close(jc, 2 * jv - 3 * jw, 1e-12 if npdt == np.float64 else 1e-5, "linearity")
    # rejected points (outside every grid) with NaN tangents add nothing
    pts, rot, trans, bg, ow, pw = args
    far = torch.full((7, n_in), 9.0, dtype=tdt, device=dev)
    pts2 = torch.cat([pts, far])
    pw2 = torch.cat([pw, torch.ones(7, dtype=tdt, device=dev)])
    nan = lambda t, shape: torch.cat([t, torch.full(shape, float("nan"), dtype=tdt, device=dev)], dim=-2
                                     if len(shape) == 3 else -1)
    kw2 = dict(kw)
    kw2["points_dot"] = nan(kw["points_dot"], (2, 7, n_in))
    kw2["point_weight_dot"] = nan(torch.zeros(2, 3000, dtype=tdt, device=dev), (2, 7))
    kw1 = dict(kw)
    kw1["point_weight_dot"] = torch.zeros(2, 3000, dtype=tdt, device=dev)
    r2 = dpr_amd.raster_jvp(pr.grid, pts2, rot, trans, bg, ow, pw2, **kw2, tangents=2, algo=algo)
    r1 = dpr_amd.raster_jvp(pr.grid, pts, rot, trans, bg, ow, pw, **kw1, tangents=2, algo=algo)
    assert bool(torch.isfinite(r2).all())
    assert_close(r2, r1, 1e-12 if npdt == np.float64 else 1e-6, "rejected points")


# ------------------------------------------------------------------ 6. raster_ad under forward_ad
def test_raster_ad_forward_mode_tiled_fp32_is_bit_identical(dev):
    pr = Problem(dev, np.float32, torch.float32, 3, 3, None, 1, P=5000, grid_n=32)
    args = pr.primal()
    tk = pr.tangent_kwargs(k=0)
    want = dpr_amd.raster_jvp(pr.grid, *args, **tk, algo="tiled")
    with fwAD.dual_level():
        duals = [fwAD.make_dual(a, tk[n + "_dot"].reshape(a.shape)) for a, n in zip(args, KINDS)]
        out = dpr_amd.raster_ad(pr.grid, *duals, algo="tiled")
        tangent = fwAD.unpack_dual(out).tangent
    assert torch.equal(tangent, want)
    # a batch on AUTO: the caller's algorithm has no JVP (chunked) or is auto -- rounding level
    pb = Problem(dev, np.float32, torch.float32, 3, 2, 4, 1, P=5000, grid_n=64)
    args = pb.primal()
    tk = pb.tangent_kwargs(k=0)
    for algo in ("auto", "chunked", "atomic"):
        with fwAD.dual_level():
            duals = [fwAD.make_dual(a, tk[n + "_dot"].reshape(a.shape)) for a, n in zip(args, KINDS)]
            tangent = fwAD.unpack_dual(dpr_amd.raster_ad(pb.grid, *duals, algo=algo)).tangent
        assert_close(tangent, dpr_amd.raster_jvp(pb.grid, *args, **tk), 1e-5, algo)


def test_raster_ad_forward_mode_equals_reverse_mode_jacobian(dev):
    pr = Problem(dev, np.float64, torch.float64, 3, 2, 2, 1, P=20, grid_n=8)
    args = [a.clone() for a in pr.primal()]
    tk = pr.tangent_kwargs(k=0)
    tangents = [tk[n + "_dot"].reshape(a.shape) for a, n in zip(args, KINDS)]
    f = lambda *xs: dpr_amd.raster_ad(pr.grid, *xs, algo="atomic")
    J = torch.autograd.functional.jacobian(f, tuple(args))
    n_out_cells = int(np.prod(pr.grid)) * 2
    jv = sum(Ji.reshape(n_out_cells, -1) @ t.reshape(-1) for Ji, t in zip(J, tangents))
    with fwAD.dual_level():
        duals = [fwAD.make_dual(a, t) for a, t in zip(args, tangents)]
        tangent = fwAD.unpack_dual(f(*duals)).tangent
    assert_close(tangent.reshape(-1), jv, 1e-12, "forward vs reverse")
    # the reverse mode is unchanged: raster_ad's gradients equal raster_pullback_
    req = [a.clone().requires_grad_(True) for a in args]
    u = dpr_amd.to_grid_layout(torch.randn(tuple(pr.grid) + (2,), dtype=torch.float64, device=dev))
    (f(*req) * u).sum().backward()
    pb = dpr_amd.raster_pullback_(u, *args, algo="atomic")
    for r, g in zip(req, pb):
        assert_close(r.grad, g.reshape(r.shape), 1e-12, "reverse mode")


# ------------------------------------------------------------------ 7. errors leave out_dot untouched
def test_errors_leave_out_dot_untouched(dev):
    pr = Problem(dev, np.float32, torch.float32, 2, 3, 2, 2, P=500, grid_n=16)
    args = pr.primal()
    kw = pr.tangent_kwargs()
    out = dpr_amd.empty_channel_grid(pr.grid, 2, 2, torch.float32, dev)
    out.fill_(7.0)
    for algo in ("tiled", "chunked"):  # (2, 3) has no tiled path; there is no chunked JVP
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.raster_jvp_(out, *args, **kw, tangents=2, algo=algo)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.raster_jvp_(out, *args, points_dot=kw["points_dot"][:, :10], tangents=2)
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.raster_jvp_(out, *args, **kw, tangents=3)
    with pytest.raises(RuntimeError):
        dpr_amd.raster_jvp_(out, *args, points_dot=kw["points_dot"].cpu(), tangents=2)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ 8. full size
def test_full_size_c3_tiled_atomic_and_adjoint(dev):
    rng = np.random.default_rng(11)
    P = 10_000_000
    pts = torch.as_tensor(0.4 * rng.normal(size=(P, 3)), dtype=torch.float32, device=dev)
    rot = torch.as_tensor(D.random_rotations(rng, 1)[0], dtype=torch.float32, device=dev)
    trans = torch.as_tensor(0.1 * rng.normal(size=3), dtype=torch.float32, device=dev)
    pw = torch.rand(P, dtype=torch.float32, device=dev)
    grid = (256,) * 3
    tk = dict(points_dot=torch.randn(P, 3, device=dev), rotation_dot=torch.randn(3, 3, device=dev),
              translation_dot=torch.randn(3, device=dev), point_weight_dot=torch.randn(P, device=dev))
    t = dpr_amd.raster_jvp(grid, pts, rot, trans, None, 2.0, pw, **tk, algo="tiled")
    a = dpr_amd.raster_jvp(grid, pts, rot, trans, None, 2.0, pw, **tk, algo="atomic")
    assert_close(t, a, 1e-5, "10M C3 tiled vs atomic")
    u = dpr_amd.to_grid_layout(torch.randn(grid, device=dev))
    g = dpr_amd.raster_pullback_(u, pts, rot, trans, None, 2.0, pw)
    lhs = float((t.double() * u.double()).sum())
    rhs = (float((tk["points_dot"].double() * g.points.double()).sum())
           + float((tk["rotation_dot"].double() * g.rotation.double()).sum())
           + float((tk["translation_dot"].double() * g.translation.double()).sum())
           + float((tk["point_weight_dot"].double() * g.point_weight.double()).sum()))
    assert abs(lhs - rhs) <= 1e-4 * float(t.double().norm() * u.double().norm()), (lhs, rhs)


def test_full_size_pose_jacobian_512sq_8_poses(dev):
    rng = np.random.default_rng(12)
    P, B, K = 1_000_000, 8, 12
    d = D.make(n_points=16, n_in=3, n_out=2, batch=B, grid_n=512, seed=12)
    pts = torch.as_tensor(0.4 * rng.normal(size=(P, 3)), dtype=torch.float32, device=dev)
    rot = torch.as_tensor(d.rotations, dtype=torch.float32, device=dev)
    trans = torch.as_tensor(d.translations, dtype=torch.float32, device=dev)
    rd = torch.randn(K, B, 2, 3, device=dev)
    td = torch.randn(K, B, 2, device=dev)
    out = dpr_amd.raster_jvp((512, 512), pts, rot, trans, rotation_dot=rd, translation_dot=td, tangents=K)
    assert tuple(out.shape) == (512, 512, K, B)
    for k in range(K):
        one = dpr_amd.raster_jvp((512, 512), pts, rot, trans, rotation_dot=rd[k], translation_dot=td[k])
        assert_close(out[..., k, :], one, 1e-6, f"pose tangent {k}")
