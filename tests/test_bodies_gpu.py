"""Rigid bodies on the GPU (dpr_raster_bodies_ex_*, dpr_raster_pullback_bodies_ex_*; kernels: csrc/dpr_kernels_bodies.h).

The ground truth is tests/bodies_reference.py, the oracle composed per body.  Tolerances are those of
tests/test_clouds_gpu.py, which are tests/test_parity_gpu.py's: fp64 1e-10 everywhere; fp32 5e-5 for `out`, 1e-4 for the
per-point gradients, 1e-3 for the per-pose and per-body sums, all norm-wise -- the pose gradients per (image, body)."""
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import bodies_reference as ref
from tests import data as D

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
NAMES = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
GRID = {2: (16, 12), 3: (16, 12, 10)}


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


@functools.lru_cache(maxsize=None)
def cloud(n_in, n_out, B, P, K, grid=None, seed=0, faces=True):
    """One cloud of P points in K bodies in random order, built like `clouds` of tests/test_clouds_gpu.py: a few points
    outside the grid, pose (0, 0) the identity with points of body 0 on cell faces, uneven weights.  (Cached: the
    arrays are shared between tests and left unchanged.)"""
    rng = np.random.default_rng(seed)
    grid = GRID[n_out] if grid is None else tuple(grid)
    d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=max(B, 1) * K, grid_n=grid, seed=seed)
    rot = d.rotations.reshape(-1, K, n_out, n_in)[:B].copy()
    trans = d.translations.reshape(-1, K, n_out)[:B].copy()
    pts = (0.15 + 0.4 * rng.uniform()) * rng.normal(size=(P, n_in))
    far = P // 50
    pts[:far] *= 6.0  # outside the grid
    body = rng.integers(0, K, size=P)
    k = min(P // 10, 64) if faces else 0
    if B * K > 0 and k:
        rot[0, 0] = np.eye(n_out, n_in)
        trans[0, 0] = 0.0
        body[far:far + k] = 0
        for j in range(min(n_in, n_out)):
            pts[far:far + k, j] = -1.0 + 2.0 * rng.integers(0, grid[j] + 1, size=k) / grid[j]
    c = dict(grid=grid, points=pts, body=body, rot=rot, trans=trans, pw=rng.uniform(0.5, 1.5, size=P),
             bg=np.arange(1, B + 1, dtype=np.float64), ow=rng.uniform(1, 10, size=B),
             ds=rng.normal(size=grid + (B,)), B=B, P=P, K=K)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def on(dev, tdt, c):
    to = lambda a: torch.as_tensor(np.array(a), device=dev).to(tdt)  # (a copy: the cached arrays are read-only)
    t = {k: to(c[k]) for k in ("points", "rot", "trans", "pw", "bg", "ow")}
    t["body"] = torch.as_tensor(np.array(c["body"]), device=dev)  # int64
    t["ds"] = dpr_amd.to_grid_layout(to(c["ds"]))
    return t


def reference(c, npdt):
    out = ref.raster(c["grid"], c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], dtype=npdt)
    pb = ref.raster_pullback(c["ds"], c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"], dtype=npdt)
    return out, pb


def run(t, c, **kw):
    args = (t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    out = dpr_amd.raster_bodies(c["grid"], *args, **kw)
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], *args, **kw)
    torch.cuda.synchronize()
    return out, pb


def check(out, pb, want_out, want_pb, npdt, what=""):
    assert_close(out, want_out, tol(npdt, "out"), f"{what}out")
    assert_close(pb.points, want_pb.points, tol(npdt, "points"), f"{what}ds_dpoints")
    assert_close(pb.point_weight, want_pb.point_weight, tol(npdt, "points"), f"{what}ds_dpoint_weight")
    B, K = want_pb.rotation.shape[:2]
    assert tuple(pb.rotation.shape) == want_pb.rotation.shape
    assert tuple(pb.translation.shape) == want_pb.translation.shape
    rot, trans = pb.rotation.cpu().numpy(), pb.translation.cpu().numpy()
    for b in range(B):
        for k in range(K):
            assert_close(rot[b, k], want_pb.rotation[b, k], tol(npdt, "pose"), f"{what}ds_drotation[{b}, {k}]")
            assert_close(trans[b, k], want_pb.translation[b, k], tol(npdt, "pose"), f"{what}ds_dtranslation[{b}, {k}]")
        assert_close(pb.background[b:b + 1], want_pb.background[b:b + 1], tol(npdt, "pose"), f"{what}ds_dbackground[{b}]")
        assert_close(pb.out_weight[b:b + 1], want_pb.out_weight[b:b + 1], tol(npdt, "pose"), f"{what}ds_dout_weight[{b}]")


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_matches_the_oracle_composed_per_body(dev, n_in, n_out, npdt, tdt):
    c = cloud(n_in, n_out, B=5, P=1999, K=3, seed=n_in * 10 + n_out)
    out, pb = run(on(dev, tdt, c), c)
    assert out.shape == c["grid"] + (5,) and out.dtype == tdt
    assert pb.rotation.shape == (5, 3, n_out, n_in) and pb.rotation.transpose(-1, -2).is_contiguous()
    check(out, pb, *reference(c, npdt), npdt)


# ------------------------------------------------------------------ 2. K = 1 is `raster`
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_one_body_one_image_stores_the_bits_of_the_atomic_pullback(dev, n_in, n_out, npdt, tdt):
    """One thread adds one pose's terms in the same order as k_bwd_gather."""
    c = cloud(n_in, n_out, B=1, P=5000, K=1, grid=(24,) * n_out, seed=3)
    t = on(dev, tdt, c)
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"],
                                         t["pw"])
    p1 = dpr_amd.raster_pullback_(t["ds"], t["points"], t["rot"][:, 0], t["trans"][:, 0], t["bg"], t["ow"], t["pw"],
                                  algo="atomic")
    torch.cuda.synchronize()
    assert torch.equal(pb.points, p1.points)
    assert torch.equal(pb.point_weight, p1.point_weight)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_one_body_three_images_is_raster(dev, n_in, n_out, npdt, tdt):
    c = cloud(n_in, n_out, B=3, P=1999, K=1, seed=4)
    t = on(dev, tdt, c)
    out, pb = run(t, c)
    poses = (t["points"], t["rot"][:, 0], t["trans"][:, 0], t["bg"], t["ow"], t["pw"])
    o1 = dpr_amd.raster(c["grid"], *poses, algo="atomic")
    p1 = dpr_amd.raster_pullback_(t["ds"], *poses, algo="atomic")
    torch.cuda.synchronize()
    assert_close(out, o1.cpu().numpy(), tol(npdt, "out"), "out")
    for name, kind in zip(NAMES, ("points", "pose", "pose", "pose", "pose", "points")):
        got = getattr(pb, name)
        got = got[:, 0] if name in ("rotation", "translation") else got
        assert_close(got, getattr(p1, name).cpu().numpy(), tol(npdt, kind), name)


# ------------------------------------------------------------------ 3. mixed waves
def by_body(c):
    order = np.argsort(c["body"], kind="stable")
    s = dict(c)
    s.update(points=c["points"][order], body=c["body"][order], pw=c["pw"][order])
    return s, order


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_mixed_waves_and_the_same_cloud_sorted_by_body(dev, n_in, n_out, npdt, tdt):
    """P = 257: one full block and a tail of one.  K = 70 random bodies: every wave walks dozens of bodies
    (csrc/dpr_kernels_bodies.h), and several bodies stay empty.  Sorted by body a wave still holds a dozen bodies of
    three or four points."""
    c = cloud(n_in, n_out, B=3, P=257, K=70, seed=5)
    empty = np.setdiff1d(np.arange(70), c["body"])
    assert len(empty) >= 2 and len(np.unique(c["body"][:64])) > 16
    want_out, want_pb = reference(c, npdt)
    out, pb = run(on(dev, tdt, c), c)
    check(out, pb, want_out, want_pb, npdt, "shuffled: ")
    s, order = by_body(c)
    assert (np.diff(s["body"]) >= 0).all() and len(np.unique(s["body"][:64])) > 1
    out_s, pb_s = run(on(dev, tdt, s), s)
    check(out_s, pb_s, *reference(s, npdt), npdt, "sorted: ")
    # ... and each other
    assert_close(out_s, out.cpu().numpy(), tol(npdt, "out"), "out, sorted against shuffled")
    assert_close(pb_s.points, pb.points.cpu().numpy()[order], tol(npdt, "points"), "ds_dpoints")
    assert_close(pb_s.point_weight, pb.point_weight.cpu().numpy()[order], tol(npdt, "points"), "ds_dpoint_weight")
    for name in ("rotation", "translation", "out_weight"):
        assert_close(getattr(pb_s, name), getattr(pb, name).cpu().numpy(), tol(npdt, "pose"), name)
    for p in (pb, pb_s):
        assert (p.rotation[:, empty] == 0).all() and (p.translation[:, empty] == 0).all()


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("order", ["random", "sorted"])
def test_a_few_bodies_per_wave(dev, n_in, n_out, npdt, tdt, order):
    """K = 5 in random order: every wave walks its five bodies.  Sorted by body: waves of one body, which reduce
    alone because their block holds two or three bodies, and waves across a boundary, which walk two.  700 points: two
    full blocks and a part of a third."""
    c = cloud(n_in, n_out, B=3, P=700, K=5, seed=6)
    if order == "sorted":
        c, _order = by_body(c)
        per_wave = [len(np.unique(c["body"][i:i + 64])) for i in range(0, 700, 64)]
        assert 1 in per_wave and 2 in per_wave and len(np.unique(c["body"][:256])) > 1
    out, pb = run(on(dev, tdt, c), c)
    check(out, pb, *reference(c, npdt), npdt)


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_one_point(dev, npdt, tdt):
    c = cloud(3, 2, B=3, P=1, K=70, seed=7, faces=False)
    out, pb = run(on(dev, tdt, c), c)
    check(out, pb, *reference(c, npdt), npdt)
    others = np.setdiff1d(np.arange(70), c["body"])
    assert (pb.rotation[:, others] == 0).all() and (pb.translation[:, others] == 0).all()


# ------------------------------------------------------------------ 4. many more bodies than points
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_many_more_bodies_than_points(dev, npdt, tdt):
    c = cloud(3, 2, B=3, P=3000, K=5000, seed=8)
    t = on(dev, tdt, c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev, dtype=tdt)
    d_rot, d_trans = nan(3, 5000, 3, 2).transpose(-1, -2), nan(3, 5000, 2)
    args = (t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    out = dpr_amd.raster_bodies(c["grid"], *args)
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], *args, ds_drotation=d_rot, ds_dtranslation=d_trans)
    torch.cuda.synchronize()
    assert pb.rotation is not None and pb.translation is d_trans
    assert not torch.isnan(pb.rotation).any() and not torch.isnan(pb.translation).any()
    check(out, pb, *reference(c, npdt), npdt)
    empty = np.setdiff1d(np.arange(5000), c["body"])
    assert len(empty) > 2000 and (pb.rotation[:, empty] == 0).all() and (pb.translation[:, empty] == 0).all()


# ------------------------------------------------------------------ 5. both sides of the pullback's launch-shape switch
@pytest.mark.parametrize("P,sliced", [(524_289, False), (1999, True)])
def test_both_sides_of_the_pose_slices(dev, P, sliced):
    """pose_slices (csrc/dpr_api.hip) cuts the images into slices while P needs fewer than 2048 blocks of 256 points:
    2049 blocks are one launch over both images with plain stores of ds_dpoints, 8 blocks two slices with float
    atomics onto zeroed buffers."""
    assert ((P + 255) // 256 < 2048) == sliced
    c = cloud(3, 2, B=2, P=P, K=3, grid=(32, 32), seed=9)
    t = on(dev, torch.float32, c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    args = (t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    out = dpr_amd.raster_bodies(c["grid"], *args)
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], *args, ds_dpoints=nan(P, 3), ds_dpoint_weight=nan(P))
    torch.cuda.synchronize()
    check(out, pb, *reference(c, np.float32), np.float32)


# ------------------------------------------------------------------ 6. drops
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("body_dtype", [torch.int32, torch.int64])
def test_dropped_points(dev, n_in, n_out, npdt, tdt, body_dtype):
    base = cloud(n_in, n_out, B=3, P=600, K=4, seed=10)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    bad_body = np.arange(100, 130)
    c["body"][bad_body] = np.resize([-1, 4, 2**31 - 1, -(2**31), 5, -7], 30)
    if body_dtype == torch.int64:  # beyond int32: still outside [0, K) after the narrowing
        c["body"][bad_body[:3]] = (2**32 + 1, -(2**32) + 2, 2**40)
    bad_pts = np.arange(300, 320)
    c["points"][bad_pts[:10], 0] = np.nan
    c["points"][bad_pts[10:15], n_in - 1] = np.inf
    c["points"][bad_pts[15:], 1] = -np.inf
    dropped = np.concatenate([bad_body, bad_pts])
    keep = np.setdiff1d(np.arange(600), dropped)
    t = on(dev, tdt, c)
    t["body"] = t["body"].to(body_dtype)
    out, pb = run(t, c)
    assert torch.isfinite(out).all()
    for x in pb:
        assert torch.isfinite(x).all()
    assert (pb.points[dropped] == 0).all() and (pb.point_weight[dropped] == 0).all()
    rest = dict(c, points=c["points"][keep], body=c["body"][keep], pw=c["pw"][keep])
    want_out, want_pb = reference(rest, npdt)
    full = lambda a: np.concatenate([a, np.zeros((len(dropped),) + a.shape[1:], a.dtype)])[
        np.argsort(np.concatenate([keep, dropped]))]
    want_pb = want_pb._replace(points=full(want_pb.points), point_weight=full(want_pb.point_weight))
    check(out, pb, want_out, want_pb, npdt)


# ------------------------------------------------------------------ 7. empty and prefilled calls
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("P,B", [(0, 3), (600, 0), (0, 0), (600, 3)])
def test_empty_calls_and_outputs_prefilled_with_nan(dev, n_in, n_out, P, B):
    K = 4
    c = cloud(n_in, n_out, B=B, P=P, K=K, seed=11, faces=False)
    t = on(dev, torch.float32, c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out = dpr_amd.empty_grid(c["grid"], B, torch.float32, dev).fill_(float("nan"))
    bufs = dict(ds_dpoints=nan(P, n_in), ds_drotation=nan(B, K, n_in, n_out).transpose(-1, -2),
                ds_dtranslation=nan(B, K, n_out), ds_dbackground=nan(B), ds_dout_weight=nan(B), ds_dpoint_weight=nan(P))
    args = (t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    assert dpr_amd.raster_bodies_(out, *args) is out
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], *args, **bufs)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    for name, x in zip(NAMES, pb):
        assert x is bufs["ds_d" + name] or name == "rotation", name
        assert not torch.isnan(x).any(), name
    assert pb.rotation.data_ptr() == bufs["ds_drotation"].data_ptr()
    if P == 0 or B == 0:
        assert torch.equal(out, t["bg"].expand(out.shape))
        for name in ("points", "rotation", "translation", "out_weight", "point_weight"):
            assert (getattr(pb, name) == 0).all(), name
        assert_close(pb.background, c["ds"].sum(axis=tuple(range(n_out))), 1e-4, "ds_dbackground")
    else:
        check(out, pb, *reference(c, np.float32), np.float32)


def test_point_weight_grad_false_returns_none_and_writes_nothing(dev):
    c = cloud(3, 2, B=3, P=600, K=4, seed=11, faces=False)
    t = on(dev, torch.float32, c)
    args = (t["points"], t["body"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    full = dpr_amd.raster_pullback_bodies_(t["ds"], *args)
    pb = dpr_amd.raster_pullback_bodies_(t["ds"], *args, point_weight_grad=False)
    torch.cuda.synchronize()
    assert pb.point_weight is None
    _out, want_pb = reference(c, np.float32)
    assert_close(pb.points, want_pb.points, 1e-4, "ds_dpoints")
    assert_close(pb.rotation, want_pb.rotation, 1e-3, "ds_drotation")
    assert_close(full.point_weight, want_pb.point_weight, 1e-4, "ds_dpoint_weight")
    with pytest.raises(ValueError):
        dpr_amd.raster_pullback_bodies_(t["ds"], *args, point_weight_grad=False, ds_dpoint_weight=torch.empty_like(t["pw"]))
    # the C entry point with the flag: the buffer it is handed stays as it was
    import ctypes

    from dpr_amd import _lib
    L = dpr_amd.lib()
    sentinel = torch.full((600,), 7.0, device=dev)
    grid = np.asarray(c["grid"], dtype=np.int64)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rot_cm = t["rot"].transpose(-1, -2).contiguous()
    body = t["body"].to(torch.int32)
    outs = [torch.empty(s, device=dev) for s in ((600, 3), (3, 4, 3, 2), (3, 4, 2), (3,), (3,))]
    rc = L.dpr_raster_pullback_bodies_ex_f32(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), _lib.ALGO_AUTO, _lib.FLAG_NO_POINT_WEIGHT_GRAD, 3, 2,
        grid.ctypes.data_as(ctypes.c_void_p), 600, 3, 4, p(t["ds"]), p(t["points"]), p(body), p(rot_cm), p(t["trans"]),
        p(t["ow"]), p(t["pw"]), *map(p, outs), p(sentinel), None, 0)
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert (sentinel == 7.0).all()
    assert_close(outs[0], want_pb.points, 1e-4, "ds_dpoints through the C entry point")


# ------------------------------------------------------------------ 8. autograd
@pytest.mark.parametrize("single", [True, False])
def test_gradcheck_raster_bodies_ad(dev, single):
    """The settings of test_gradcheck_raster_clouds_ad; the cloud is kept off the cell faces (no kinks under the
    differences)."""
    c = cloud(3, 2, B=1 if single else 2, P=30, K=3, grid=(8, 8), seed=15, faces=False)
    t = on(dev, torch.float64, c)
    pick = (lambda x: x[0]) if single else (lambda x: x)
    args = [t["points"].clone().requires_grad_(), pick(t["rot"]).clone().requires_grad_(),
            pick(t["trans"]).clone().requires_grad_(), pick(t["bg"]).clone().requires_grad_(),
            pick(t["ow"]).clone().requires_grad_(), t["pw"].clone().requires_grad_()]
    fn = lambda pts, R, tr, bg, ow, w: dpr_amd.raster_bodies_ad(c["grid"], pts, t["body"], R, tr, bg, ow, w)
    assert fn(*args).shape == ((8, 8) if single else (8, 8, 2))
    assert torch.autograd.gradcheck(fn, tuple(args), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=1e-12)


# ------------------------------------------------------------------ 9. stream contract
class Calls:
    """Forward and pullback on device buffers that stay where they are (the pattern of
    tests/test_families_streams_gpu.py)."""
    B, P, K = 3, 1999, 5

    def __init__(self, dev):
        self.dev = dev
        self.inp = on(dev, torch.float32, self.problem(0))
        self.body32 = self.inp["body"].to(torch.int32)  # (narrowed here: the calls then make no copy of it)
        g = self.problem(0)["grid"]
        B, P, K = self.B, self.P, self.K
        e = lambda *s: torch.empty(s, device=dev)
        self.out = dpr_amd.empty_grid(g, B, torch.float32, dev)
        self.grads = dict(ds_dpoints=e(P, 3), ds_drotation=e(B, K, 3, 3).transpose(-1, -2), ds_dtranslation=e(B, K, 3),
                          ds_dbackground=e(B), ds_dout_weight=e(B), ds_dpoint_weight=e(P))
        self.staged = {}

    def problem(self, seed):
        return cloud(3, 3, B=self.B, P=self.P, K=self.K, seed=40 + seed)

    def floats(self):
        return [v for k, v in self.inp.items() if k != "body"]

    def poison(self):
        for v in self.floats():
            v.fill_(float("nan"))
        self.body32.fill_(-1)
        self.poison_outputs()

    def poison_outputs(self):
        self.out.fill_(float("nan"))
        for v in self.grads.values():
            v.fill_(float("nan"))

    def stage(self, *seeds):
        for seed in seeds:
            s = on(self.dev, torch.float32, self.problem(seed))
            s["body"] = s["body"].to(torch.int32)
            self.staged[seed] = s
        torch.cuda.synchronize()

    def load(self, seed):
        for k, v in self.inp.items():
            (self.body32 if k == "body" else v).copy_(self.staged[seed][k], non_blocking=True)

    def run(self):
        i = self.inp
        args = (i["points"], self.body32, i["rot"], i["trans"], i["bg"], i["ow"], i["pw"])
        dpr_amd.raster_bodies_(self.out, *args)
        self.pb = dpr_amd.raster_pullback_bodies_(i["ds"], *args, **self.grads)

    def check(self, seed, what):
        check(self.out, self.pb, *reference(self.problem(seed), np.float32), np.float32, what + ": ")


def filler(dev):
    a = torch.randn(4096, 4096, device=dev)
    b = torch.empty_like(a)
    return lambda: [torch.matmul(a, a, out=b) for _ in range(4)]  # (a few milliseconds on the stream it is called on)


def test_runs_on_the_callers_stream(dev):
    """The inputs start as NaN (body: -1); on a side stream a filler, the copies of the real inputs, the calls.  A
    launch or zeroing on another stream would not wait for them.  (Can pass by luck of timing, never fail by it.)"""
    c = Calls(dev)
    c.poison()
    c.stage(0)
    busy = filler(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        busy()
        c.load(0)
        c.run()
    side.synchronize()
    c.check(0, "side stream")


def test_is_captured_into_a_hip_graph_and_replayed_on_new_contents(dev):
    c = Calls(dev)
    c.stage(0, 2)
    c.load(0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c.run()  # warm-up outside the capture
    side.synchronize()
    c.check(0, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one stream, no fork
        c.run()
    for seed, what in ((2, "graph replay on new contents"), (0, "second replay, on the first contents")):
        c.load(seed)
        c.poison_outputs()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        c.check(seed, what)
