"""Forward-mode derivative of the smooth splat of rigid bodies on the GPU (dpr_raster_smooth_bodies_jvp_ex_*,
raster_smooth_bodies_jvp, raster_smooth_bodies_ad under forward_ad; include/dpr.h, SMOOTH SPLAT, RIGID BODIES, FORWARD
MODE; kernels: csrc/dpr_smooth_bodies.hip) against the fp64 numpy reference tests/smooth_bodies_jvp_reference.py, the
library's own pullback, forward and single-body JVP.

Shapes: those of tests/test_smooth_bodies_gpu.py (_case, GRIDS, SMALL): grids (70, 19) and (18, 9, 10) -- 2 x 2 and
2 x 2 x 2 tiles, no axis a multiple of its tile -- and (5, 7), smaller than a tile; clouds with points planted at
j0 = -1 and j0 = n of every axis and points accepted in one image and rejected in another.  The base case is
sizes = (300, 200, 0, 277): P = 777, K = 4 with one empty body, B = 3, V = 2 -- B, K and V differ pairwise, so a swapped
index fails -- in the sorted and the shuffled order.  Inputs are rounded to fp32 once, so one fp64 reference serves
both dtypes; rotation_dot is not symmetric.

Tolerances, norm-wise per plane: against the reference 1e-10 fp64 / 1e-4 fp32 (tests/test_smooth_jvp_gpu.py's); one
library call against another (tiled / auto against atomic, linearity, NULL against zero tangents, V = 16 against single
calls, composition, forward mode) 1e-12 / 1e-5."""
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import dpr_amd
from tests import smooth_bodies_jvp_reference as BJR
from tests.test_parity_gpu import T, grid_to_dev
from tests.test_smooth_bodies_gpu import GRIDS, SMALL, _accepted, _case
from tests.test_smooth_bodies_jvp_reference import SIZES, tangents as _tangents
from tests.test_smooth_clouds_gpu import _cloud, _coords, _poses
from tests.test_smooth_jvp_gpu import assert_close, tol

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
ALGOS = ("atomic", "tiled")
KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
V = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def primal(n_in, n_out, grid=None, sizes=SIZES, B=3, order="sorted", seed=2):
    """A case of tests/test_smooth_bodies_gpu.py with its values rounded to fp32 (exact in either dtype)."""
    c = _case(n_in, n_out, grid=grid, sizes=sizes, B=B, order=order, seed=seed)
    p = {k: _r32(c[k]) for k in ("points", "rot", "trans", "bg", "ow", "pw", "g")}
    p.update(grid=c["grid"], body=np.array(c["body"]), B=c["B"], K=c["K"], P=c["P"],
             key=(n_in, n_out, grid, sizes, B, order, seed))  # (primal(*key) is this case)
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def tangents(key, n_tangents=V, seed=0):
    """All six tangents ~ N(0, 1) with a leading axis of n_tangents, rounded to fp32, by their KINDS name."""
    t = _tangents(primal(*key), n_tangents, seed)
    return _frozen({k: _r32(t[k + "_dot"]) for k in KINDS})


def numpy_jvp(p, t, n_tangents, kinds=KINDS, body=None, keep=slice(None)):
    tan = {k + "_dot": (t[k][:, keep] if k in ("points", "point_weight") else t[k]) for k in kinds}
    body = p["body"] if body is None else body
    return BJR.raster_smooth_bodies_jvp(p["grid"], p["points"][keep], body[keep], p["rot"], p["trans"], p["ow"],
                                        p["pw"][keep], V=n_tangents, **tan)


@functools.lru_cache(maxsize=None)
def reference(key, n_tangents=V, kinds=KINDS, seed=0):
    out = numpy_jvp(primal(*key), tangents(key, n_tangents, seed), n_tangents, kinds)
    out.setflags(write=False)
    return out


def dev_primal(p, dev, npdt, body_dtype=torch.int64):
    """points, body, rotation, translation, background, out_weight, point_weight"""
    f = lambda k: T(p[k].astype(npdt), dev)
    return [f("points"), torch.as_tensor(np.array(p["body"]), device=dev).to(body_dtype), f("rot"), f("trans"),
            f("bg"), f("ow"), f("pw")]


def dev_tangents(t, dev, npdt, kinds=KINDS, v=None):
    """tangents=V form; `v`: tangent v alone in the tangents=None form"""
    return {k + "_dot": T((t[k] if v is None else t[k][v]).astype(npdt), dev) for k in kinds}


def jvp(p, t, dev, npdt, n_tangents, algo, kinds=KINDS, **kw):
    return dpr_amd.raster_smooth_bodies_jvp(p["grid"], *dev_primal(p, dev, npdt), **dev_tangents(t, dev, npdt, kinds),
                                            tangents=n_tangents, algo=algo, **kw)


def planes_close(out, want, rtol, what):
    """norm-wise per plane (v, b)"""
    assert tuple(out.shape) == tuple(want.shape), f"{what}: shape {tuple(out.shape)} != {tuple(want.shape)}"
    for v in range(out.shape[-2]):
        for b in range(out.shape[-1]):
            assert_close(out[..., v, b], want[..., v, b], rtol, f"{what} plane ({v}, {b})")


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("kinds", [KINDS] + [(k,) for k in KINDS], ids=lambda k: "all" if len(k) > 1 else k[0])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_matches_the_reference(dev, n_in, n_out, order, kinds):
    grids = [None] + ([SMALL] if n_out == 2 and len(kinds) > 1 else [])
    for grid in grids:
        p = primal(n_in, n_out, grid=grid, order=order)
        assert (p["P"], p["K"], p["B"]) == (777, 4, 3) and 2 not in p["body"]
        assert (np.diff(p["body"]) >= 0).all() == (order == "sorted")
        t = tangents(p["key"])
        if n_in == n_out:  # (a row-major read of rotation_dot fails)
            assert not np.allclose(t["rotation"], np.swapaxes(t["rotation"], -1, -2))
        ref = reference(p["key"], V, kinds)
        for v in range(V):
            for b in range(3):
                assert np.linalg.norm(ref[..., v, b]) > 0
        for npdt, tdt in DTYPES:
            for algo in ALGOS + ("auto",):
                out = jvp(p, t, dev, npdt, V, algo, kinds)
                assert tuple(out.shape) == p["grid"] + (V, 3) and out.dtype == tdt
                planes_close(out, ref, tol(npdt), f"{p['grid']} {algo} {npdt.__name__} {order} {kinds}")


def test_the_case_reaches_the_branches_it_is_drawn_for():
    """(no device) planted points at j0 = -1 and j0 = n, points accepted in one image and rejected in another"""
    for n_in, n_out in PAIRS:
        c = _case(n_in, n_out, sizes=SIZES, seed=2)
        acc = _accepted(c)
        assert (acc.any(axis=0) & ~acc.all(axis=0)).any() and (~acc.any(axis=0)).any()
        for k in (0, 1, 3):
            idx = np.flatnonzero((c["body"] == k) & acc[0])
            j0 = np.floor(_coords(c["grid"], c["points"][idx], c["rot"][0, k], c["trans"][0, k])).astype(int)
            for d in range(n_out):
                assert (j0[:, d] == -1).any() and (j0[:, d] == c["grid"][d]).any()


# ------------------------------------------------------------------ 2. one call against another
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_and_auto_equal_atomic_and_the_jvp_is_linear(dev, npdt, tdt, n_in, n_out, order):
    p = primal(n_in, n_out, order=order)
    v, w = tangents(p["key"], V, 1), tangents(p["key"], V, 2)
    rt = tol(npdt, 1e-12, 1e-5)
    a = jvp(p, v, dev, npdt, V, "atomic")
    planes_close(jvp(p, v, dev, npdt, V, "tiled"), a, rt, "tiled vs atomic")
    assert dpr_amd.resolve_algo_smooth_bodies_jvp(p["grid"], p["P"], 3, 4, n_in, V) in ALGOS
    planes_close(jvp(p, v, dev, npdt, V, "auto"), a, rt, "auto vs atomic")
    mix = {k: 2 * v[k] - 3 * w[k] for k in KINDS}
    for algo in ALGOS:
        jv, jw = jvp(p, v, dev, npdt, V, algo), jvp(p, w, dev, npdt, V, algo)
        planes_close(jvp(p, mix, dev, npdt, V, algo), 2 * jv.double() - 3 * jw.double(), rt, f"linearity {algo}")


# ------------------------------------------------------------------ 3. NULL tangents
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_null_tangents_are_zero_tangents(dev, npdt, tdt, n_in, n_out):
    """Some tangents omitted against the same call with explicit zeros in their place: 1e-12 / 1e-5 (the deposits are
    the same bits, the order of the atomics is not).  Every tangent but background_dot omitted -- the call that
    launches no deposit kernel -- against explicit zeros: `==` on "tiled" in fp64, where a tile whose cells sum to
    exactly 0 adds nothing onto the background tangent."""
    p = primal(n_in, n_out, order="shuffled")
    t = tangents(p["key"], V, 1)
    some = ("rotation", "point_weight", "background")
    zeros = {k: (t[k] if k in some else np.zeros_like(t[k])) for k in KINDS}
    only_bg = {k: (t[k] if k == "background" else np.zeros_like(t[k])) for k in KINDS}
    for algo in ALGOS:
        planes_close(jvp(p, zeros, dev, npdt, V, algo), jvp(p, t, dev, npdt, V, algo, some), tol(npdt, 1e-12, 1e-5),
                     f"NULL vs zero, {algo}")
        null, zero = jvp(p, t, dev, npdt, V, algo, ("background",)), jvp(p, only_bg, dev, npdt, V, algo)
        want = np.broadcast_to(t["background"].astype(npdt), p["grid"] + (V, 3))
        assert np.array_equal(null.cpu().numpy(), want)
        if algo == "tiled" and npdt == np.float64:
            assert torch.equal(null, zero)
        planes_close(zero, null, tol(npdt, 1e-12, 1e-5), f"all NULL vs all zero, {algo}")
        none = dpr_amd.raster_smooth_bodies_jvp(p["grid"], *dev_primal(p, dev, npdt), tangents=V, algo=algo)
        assert not bool(none.any())


# ------------------------------------------------------------------ 4. sixteen tangents
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_sixteen_tangents_equal_sixteen_single_calls(dev, npdt, tdt, n_in, n_out, algo):
    p = primal(n_in, n_out, order="shuffled")
    t = tangents(p["key"], 16)
    out = jvp(p, t, dev, npdt, 16, algo)
    assert tuple(out.shape) == p["grid"] + (16, 3)
    args = dev_primal(p, dev, npdt)
    for v in range(16):
        single = dpr_amd.raster_smooth_bodies_jvp(p["grid"], *args, **dev_tangents(t, dev, npdt, v=v), algo=algo)
        assert tuple(single.shape) == p["grid"] + (3,)  # tangents=None: the shape of raster_smooth_bodies' result
        for b in range(3):
            assert_close(out[..., v, b], single[..., b], tol(npdt, 1e-12, 1e-5), f"{algo} plane ({v}, {b})")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_smooth_bodies_jvp(p["grid"], *args, tangents=17, algo=algo)


# ------------------------------------------------------------------ 5. NaN tangents of dropped points
@pytest.mark.parametrize("body_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_nan_tangents_of_dropped_points_leave_no_trace(dev, body_dtype, npdt, tdt, n_in, n_out):
    """NaN in every tangent of the points no image accepts and of the points whose body is -1, K, 2^31 - 1 (int64:
    also +-2^40): the result is finite and equals the call without those points."""
    p = primal(n_in, n_out, order="shuffled")
    t = tangents(p["key"])
    K = p["K"]
    c = _case(n_in, n_out, sizes=SIZES, order="shuffled", seed=2)
    never = ~_accepted(c).any(axis=0)
    # (points within 1e-3 cells of the acceptance border could flip between numpy and the device: left alone)
    n = np.asarray(p["grid"])
    for b in range(3):
        for k in range(K):
            idx = np.flatnonzero(p["body"] == k)
            co = _coords(p["grid"], p["points"][idx], p["rot"][b, k], p["trans"][b, k])
            never[idx[((np.abs(co + 1) < 1e-3) | (np.abs(co - (n + 1)) < 1e-3)).any(axis=1)]] = False
    assert never.sum() > 10
    out_of_range = np.setdiff1d(np.arange(100, 130), np.flatnonzero(never))
    body = np.array(p["body"])
    body[out_of_range] = np.resize([-1, K, 2**31 - 1], len(out_of_range))
    if body_dtype == torch.int64:
        body[out_of_range[:4]] = (2**40, -(2**40), 2**40 + 1, -(2**40) + 2)
    dropped = np.union1d(np.flatnonzero(never), out_of_range)
    keep = np.setdiff1d(np.arange(p["P"]), dropped)
    bad = {k: t[k].copy() for k in KINDS}
    bad["points"][:, dropped] = np.nan
    bad["point_weight"][:, dropped] = np.nan
    want = numpy_jvp(p, t, V, body=np.clip(body, -1, K), keep=keep)
    args = dev_primal(p, dev, npdt)
    args[1] = torch.as_tensor(body, device=dev).to(body_dtype)
    rest = [args[0][keep].contiguous(), args[1][keep].contiguous(), *args[2:6], args[6][keep].contiguous()]
    tk = {k: (t[k][:, keep] if k in ("points", "point_weight") else t[k]) for k in KINDS}
    for algo in ALGOS:
        out = dpr_amd.raster_smooth_bodies_jvp(p["grid"], *args, **dev_tangents(bad, dev, npdt), tangents=V, algo=algo)
        assert bool(torch.isfinite(out).all())
        planes_close(out, want, tol(npdt), f"{algo} against the reference without them")
        without = dpr_amd.raster_smooth_bodies_jvp(p["grid"], *rest, **dev_tangents(tk, dev, npdt), tangents=V,
                                                   algo=algo)
        planes_close(out, without, tol(npdt, 1e-12, 1e-5), f"{algo} against the call without them")


# ------------------------------------------------------------------ 6. composition of the single-body JVP
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_planes_are_the_sums_of_the_subset_calls(dev, npdt, tdt, n_in, n_out):
    """With background_dot omitted, plane (v, b) is the sum over k of raster_smooth_jvp of subset k under pose (b, k)
    with that subset's tangents."""
    p = primal(n_in, n_out, order="shuffled")
    t = tangents(p["key"])
    kinds = tuple(k for k in KINDS if k != "background")
    pts, body, rot, trans, _bg, ow, pw = dev_primal(p, dev, npdt)
    td = dev_tangents(t, dev, npdt, kinds)
    total = None
    for k in range(p["K"]):
        idx = torch.nonzero(body == k).flatten()
        one = dpr_amd.raster_smooth_jvp(
            p["grid"], pts[idx].contiguous(), rot[:, k].contiguous(), trans[:, k].contiguous(), None, ow,
            pw[idx].contiguous(), points_dot=td["points_dot"][:, idx].contiguous(),
            rotation_dot=td["rotation_dot"][:, :, k].contiguous(),
            translation_dot=td["translation_dot"][:, :, k].contiguous(), out_weight_dot=td["out_weight_dot"],
            point_weight_dot=td["point_weight_dot"][:, idx].contiguous(), tangents=V, algo="atomic")
        total = one.double() if total is None else total + one.double()
    assert float(total.abs().max()) > 0
    for algo in ALGOS:
        planes_close(jvp(p, t, dev, npdt, V, algo, kinds), total, tol(npdt, 1e-12, 1e-5), f"{algo} vs the subset calls")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_one_body_is_raster_smooth_jvp(dev, npdt, tdt, n_in, n_out):
    p = primal(n_in, n_out, sizes=(777,), seed=1)
    t = tangents(p["key"])
    pts, _body, rot, trans, bg, ow, pw = dev_primal(p, dev, npdt)
    td = dev_tangents(t, dev, npdt)
    td1 = dict(td, rotation_dot=td["rotation_dot"][:, :, 0].contiguous(),
               translation_dot=td["translation_dot"][:, :, 0].contiguous())
    want = dpr_amd.raster_smooth_jvp(p["grid"], pts, rot[:, 0].contiguous(), trans[:, 0].contiguous(), bg, ow, pw,
                                     **td1, tangents=V, algo="atomic")
    ref = reference(p["key"])
    for algo in ALGOS:
        out = jvp(p, t, dev, npdt, V, algo)
        planes_close(out, want, tol(npdt, 1e-12, 1e-5), f"{algo} vs raster_smooth_jvp")
        planes_close(out, ref, tol(npdt), f"{algo} vs the reference")


# ------------------------------------------------------------------ 7. groups of images
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_groups_of_images(dev, group, npdt, tdt, n_in, n_out):
    """B = 5: max_pose_group 1 (image by image), 2 (groups of 2 + 2 + 1) and 0 (all five images in one group), in place
    onto a buffer full of NaN."""
    p = primal(n_in, n_out, sizes=(100, 100, 100), B=5, order="shuffled", seed=4)
    t = tangents(p["key"])
    ref = reference(p["key"])
    args, td = dev_primal(p, dev, npdt), dev_tangents(t, dev, npdt)
    buf = torch.full_like(dpr_amd.empty_channel_grid(p["grid"], V, 5, tdt, dev), float("nan"))
    got = dpr_amd.raster_smooth_bodies_jvp_(buf, *args, **td, tangents=V, algo="tiled", max_pose_group=group)
    assert got is buf and bool(torch.isfinite(buf).all())
    planes_close(buf, ref, tol(npdt), f"group {group}")
    with pytest.raises(ValueError):
        dpr_amd.raster_smooth_bodies_jvp(p["grid"], *args, **td, tangents=V, algo="tiled", max_pose_group=17)


# ------------------------------------------------------------------ 8. adjoint identity with the library's pullback
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_adjoint_identity_with_the_pullback(dev, npdt, tdt, n_in, n_out, order):
    p = primal(n_in, n_out, order=order)
    t = tangents(p["key"])
    g = grid_to_dev(p["g"].astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, *dev_primal(p, dev, npdt))
    grads = [x.double().cpu().numpy() for x in pb]
    for algo in ALGOS:
        jv = jvp(p, t, dev, npdt, V, algo).double().cpu().numpy()
        for v in range(V):
            lhs = float((jv[..., v, :] * p["g"]).sum())
            rhs = sum(float((t[name][v] * grad).sum()) for name, grad in zip(KINDS, grads))
            bound = tol(npdt, 1e-11, 1e-4) * np.linalg.norm(jv[..., v, :]) * np.linalg.norm(p["g"])
            print(f"({n_in},{n_out}) {npdt.__name__} {algo} v={v}: |lhs - rhs| = {abs(lhs - rhs):.3e}, "
                  f"bound {bound:.3e}")
            assert abs(lhs - rhs) <= bound, (algo, v, lhs, rhs)


# ------------------------------------------------------------------ 9. the exact derivative, fp64
def _tiny(n_in, n_out, rng):
    """8^N grid, 2 images, 3 bodies, 12 points (the shape of tests/test_smooth_bodies_gpu.py's central differences)"""
    nb, K, npts = 2, 3, 12
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(npts, n_in)), rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out),
            rng.normal(size=nb), rng.uniform(0.5, 1.5, size=nb), rng.uniform(0.5, 1.5, size=npts)]
    return (8,) * n_out, np.arange(npts) % K, vals


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_central_differences_of_the_forward(dev, algo, n_in, n_out):
    """fp64: differences of raster_smooth_bodies along the joint tangent with step 1e-7, norm-wise within 1e-6."""
    rng = np.random.default_rng(11)
    grid, body, vals = _tiny(n_in, n_out, rng)
    tans = [rng.normal(size=v.shape) for v in vals]
    tb = torch.as_tensor(body, device=dev)
    h = 1e-7
    jv = dpr_amd.raster_smooth_bodies_jvp(grid, T(vals[0], dev), tb, *[T(v, dev) for v in vals[1:]],
                                          **{k + "_dot": T(x, dev) for k, x in zip(KINDS, tans)}, algo=algo)
    f = lambda s: dpr_amd.raster_smooth_bodies(grid, T(vals[0] + s * h * tans[0], dev), tb,
                                               *[T(v + s * h * x, dev) for v, x in zip(vals[1:], tans[1:])], algo=algo)
    fd = (f(+1) - f(-1)) / (2 * h)
    assert jv.shape == fd.shape == grid + (2,) and float(jv.abs().max()) > 0
    assert_close(jv, fd, 1e-6, f"{algo} central differences")


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_out_dot_is_continuous_across_a_cell_face(dev, algo, n_in, n_out):
    """Every point of body 1 sits 1e-9 cells either side of a cell face of axis 0 in image 1 (fp64; the clouds of
    tests/test_smooth_bodies_gpu.py's face test): out_dot of the two calls agrees within 1e-6."""
    rng = np.random.default_rng(5)
    grid, nb, K, per = (8,) * n_out, 3, 3, 6
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    rot, trans = rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out)
    pts = np.concatenate([_cloud(rng, grid, rot[1, k], trans[1, k], n_in, per, lo=1.0, hi=-1.0) for k in range(K)])
    body = np.repeat(np.arange(K), per)
    face = np.array([2, 3, 4, 5, 6, 3], dtype=np.float64)
    base = rng.uniform(1, 7, size=(per, n_out))
    tan = dict(points_dot=rng.normal(size=pts.shape), rotation_dot=rng.normal(size=rot.shape),
               translation_dot=rng.normal(size=trans.shape), point_weight_dot=rng.normal(size=len(pts)))
    outs = []
    for eps in (-1e-9, 1e-9):
        coord = base.copy()
        coord[:, 0] = face + eps
        x = pts.copy()
        x[body == 1] = ((-1 + 2 * coord / 8) - trans[1, 1]) @ rot[1, 1]
        assert np.all(np.floor(_coords(grid, x[body == 1], rot[1, 1], trans[1, 1])[:, 0]) == face + (eps > 0) - 1)
        outs.append(dpr_amd.raster_smooth_bodies_jvp(grid, T(x, dev), torch.as_tensor(body, device=dev), T(rot, dev),
                                                     T(trans, dev), algo=algo,
                                                     **{k: T(v, dev) for k, v in tan.items()}))
    assert float(outs[0][..., 1].abs().max()) > 0
    assert_close(outs[0], outs[1], 1e-6, "either side of the face")


# ------------------------------------------------------------------ 10. edge shapes
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_one_point_no_images_and_the_single_image_form(dev, algo, npdt, tdt, n_in, n_out):
    p = primal(n_in, n_out)
    t = tangents(p["key"])
    grid, B, K = p["grid"], p["B"], p["K"]
    pts, body, rot, trans, bg, ow, pw = dev_primal(p, dev, npdt)
    td = dev_tangents(t, dev, npdt)
    pose_t = {k: td[k] for k in ("rotation_dot", "translation_dot", "background_dot", "out_weight_dot")}
    # P = 0: the planes equal background_dot
    out = dpr_amd.raster_smooth_bodies_jvp(grid, pts[:0], body[:0], rot, trans, bg, ow, pw[:0], **pose_t,
                                           points_dot=td["points_dot"][:, :0], point_weight_dot=td["point_weight_dot"][:, :0],
                                           tangents=V, algo=algo)
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(t["background"].astype(npdt), grid + (V, B)))
    # P = 1 (a point of body 1 that every image accepts)
    c = _case(n_in, n_out, sizes=SIZES, seed=2)
    i = int(np.flatnonzero((p["body"] == 1) & _accepted(c).all(axis=0))[0])
    sl = slice(i, i + 1)
    want = numpy_jvp(p, t, V, keep=sl)
    out = dpr_amd.raster_smooth_bodies_jvp(grid, pts[sl].contiguous(), body[sl].contiguous(), rot, trans, bg, ow,
                                           pw[sl].contiguous(), **pose_t, points_dot=td["points_dot"][:, sl].contiguous(),
                                           point_weight_dot=td["point_weight_dot"][:, sl].contiguous(), tangents=V,
                                           algo=algo)
    assert np.abs(want - t["background"]).max() > 1e-3
    planes_close(out, want, tol(npdt), "P=1")
    # B = 0
    e = lambda *s: torch.zeros(s, dtype=tdt, device=dev)
    out = dpr_amd.raster_smooth_bodies_jvp(grid, pts, body, e(0, K, n_out, n_in), e(0, K, n_out), tangents=V, algo=algo,
                                           points_dot=td["points_dot"])
    assert out.shape == grid + (V, 0)
    out = dpr_amd.raster_smooth_bodies_jvp(grid, pts, body, e(0, K, n_out, n_in), e(0, K, n_out), algo=algo)
    assert out.shape == grid + (0,)
    # the single-image form: no B axis in any tangent nor in the result
    b = 1
    ref = reference(p["key"])
    one = (pts, body, rot[b], trans[b], float(p["bg"][b]), float(p["ow"][b]), pw)
    outV = dpr_amd.raster_smooth_bodies_jvp(
        grid, *one, points_dot=td["points_dot"], rotation_dot=td["rotation_dot"][:, b].contiguous(),
        translation_dot=td["translation_dot"][:, b].contiguous(), background_dot=td["background_dot"][:, b].contiguous(),
        out_weight_dot=td["out_weight_dot"][:, b].contiguous(), point_weight_dot=td["point_weight_dot"], tangents=V,
        algo=algo)
    assert outV.shape == grid + (V,)
    for v in range(V):
        assert_close(outV[..., v], ref[..., v, b], tol(npdt), f"single image, tangents=V, plane {v}")
    out1 = dpr_amd.raster_smooth_bodies_jvp(
        grid, *one, points_dot=td["points_dot"][1], rotation_dot=td["rotation_dot"][1, b],
        translation_dot=td["translation_dot"][1, b], background_dot=float(t["background"][1, b]),
        out_weight_dot=float(t["out_weight"][1, b]), point_weight_dot=td["point_weight_dot"][1], algo=algo)
    assert out1.shape == grid
    assert_close(out1, ref[..., 1, b], tol(npdt), "single image, tangents=None")


# ------------------------------------------------------------------ 11. raster_smooth_bodies_ad in forward mode
@pytest.mark.parametrize("algo", ["auto", "atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_mode_through_autograd(dev, npdt, tdt, n_in, n_out, algo):
    """raster_smooth_bodies_ad under forward_ad.dual_level: raises without a jvp on the autograd function."""
    p = primal(n_in, n_out, order="shuffled")
    t = tangents(p["key"], 1)
    args = dev_primal(p, dev, npdt)
    body, floats = args[1], [args[0]] + args[2:]
    tans = [T(t[k][0].astype(npdt), dev) for k in KINDS]
    want = dpr_amd.raster_smooth_bodies_jvp(p["grid"], *args, **{k + "_dot": x for k, x in zip(KINDS, tans)},
                                            algo=algo)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(a, x) for a, x in zip(floats, tans)]
        out = dpr_amd.raster_smooth_bodies_ad(p["grid"], duals[0], body, *duals[1:], algo=algo)
        primal_out, tangent = fwAD.unpack_dual(out)
    assert tangent is not None and tangent.shape == want.shape == p["grid"] + (3,)
    assert float(want.abs().max()) > 0
    assert_close(tangent, want, tol(npdt, 1e-12, 1e-5), f"forward mode, {algo}")
    assert_close(primal_out, dpr_amd.raster_smooth_bodies(p["grid"], *args, algo=algo), tol(npdt, 1e-12, 1e-5),
                 "primal")
    # torch.func.jvp, one image; only the rotation carries a tangent, the optional arguments are constants
    R, tr, Rd = args[2][1], args[3][1], tans[1][1]
    f = lambda rot: dpr_amd.raster_smooth_bodies_ad(p["grid"], args[0], body, rot, tr, None, 2.0, algo=algo)
    _out, tangent = torch.func.jvp(f, (R,), (Rd,))
    want = dpr_amd.raster_smooth_bodies_jvp(p["grid"], args[0], body, R, tr, None, 2.0, rotation_dot=Rd, algo=algo)
    assert tangent.shape == p["grid"]
    assert_close(tangent, want, tol(npdt, 1e-12, 1e-5), f"rotation tangent alone, {algo}")


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_mode_and_reverse_mode_jacobians_agree(dev, n_in, n_out):
    """The tiny fp64 case: the Jacobian of raster_smooth_bodies_ad from reverse mode against the one assembled column
    by column from dual tensors, within 1e-12 * max(1, |J|)."""
    rng = np.random.default_rng(21)
    grid, body, vals = _tiny(n_in, n_out, rng)
    tb = torch.as_tensor(body, device=dev)
    args = [torch.tensor(v, dtype=torch.float64, device=dev) for v in vals]
    f = lambda *xs: dpr_amd.raster_smooth_bodies_ad(grid, xs[0], tb, *xs[1:], algo="atomic")
    J = torch.autograd.functional.jacobian(f, tuple(args))
    cells = int(np.prod(grid)) * 2
    for i, (a, Ji) in enumerate(zip(args, J)):
        Ji = Ji.reshape(cells, -1)
        scale = float(Ji.abs().max())
        assert scale > 0
        for col in range(a.numel()):
            e = torch.zeros(a.numel(), dtype=torch.float64, device=dev)
            e[col] = 1
            with fwAD.dual_level():
                xs = list(args)
                xs[i] = fwAD.make_dual(a, e.reshape(a.shape))
                tangent = fwAD.unpack_dual(f(*xs)).tangent
            err = float((tangent.reshape(-1) - Ji[:, col]).abs().max())
            assert err <= 1e-12 * max(1.0, scale), (KINDS[i], col, err)


@pytest.mark.parametrize("algo", ["auto", "atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_reverse_mode_is_the_direct_pullback_call(dev, npdt, tdt, algo):
    """Adding `jvp` leaves `backward` as it was: the gradients are torch.equal to a direct
    raster_pullback_smooth_bodies_ call on the same inputs, as the backward makes it (a forward on "tiled"
    differentiates on "auto").  The inputs are chosen so that two identical pullback calls give the same bits: one
    image of the (5, 7) grid (one block sums the image; one slice stores the point gradients) and five accepted
    points of each of three bodies in one wave (a masked wave sum in a fixed order, then one atomic per value onto a
    zeroed buffer).  On the base case the pose sums are float atomics from several waves in arrival order."""
    p = primal(2, 2, grid=SMALL)
    acc = _accepted(_case(2, 2, grid=SMALL, sizes=SIZES, seed=2))[0]
    take = np.concatenate([np.flatnonzero((p["body"] == k) & acc)[:5] for k in (0, 1, 3)])
    assert len(take) == 15
    args = dev_primal(p, dev, npdt)
    pts, body, pw = args[0][take].contiguous(), args[1][take].contiguous(), args[6][take].contiguous()
    rot, trans, bg, ow = (a[0].contiguous() for a in args[2:6])  # image 0, the single-image form
    xs = [x.clone().requires_grad_() for x in (pts, rot, trans, bg, ow, pw)]
    g = grid_to_dev(p["g"][..., 0].astype(npdt), dev)
    out = dpr_amd.raster_smooth_bodies_ad(SMALL, xs[0], body, *xs[1:], algo=algo)
    out.backward(g)
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, pts, body, rot, trans, bg, ow, pw,
                                                algo="auto" if algo == "tiled" else algo, point_weight_grad=True)
    torch.cuda.synchronize()
    for name, x, want in zip(KINDS, xs, pb):
        assert float(want.abs().max()) > 0, name
        assert torch.equal(x.grad, want.reshape(x.shape).to(x.dtype)), name


# ------------------------------------------------------------------ 12. refused calls leave out_dot untouched
def test_refused_calls_leave_out_dot_untouched(dev):
    import ctypes

    from dpr_amd import _lib
    n_in, n_out, npdt = 3, 3, np.float32
    p = primal(n_in, n_out)
    t = tangents(p["key"])
    B, K, P = p["B"], p["K"], p["P"]
    args, td = dev_primal(p, dev, npdt), dev_tangents(t, dev, npdt)
    out = torch.full_like(dpr_amd.empty_channel_grid(p["grid"], V, B, torch.float32, dev), float("nan"))
    L = _lib.lib()
    grid = np.asarray(p["grid"], dtype=np.int64)
    gp = grid.ctypes.data_as(ctypes.c_void_p)
    need = L.dpr_workspace_bytes_smooth_bodies_jvp_ex_f32(_lib.ALGO_TILED, 0, n_in, n_out, gp, P, B, K, V)
    assert need not in (0, ctypes.c_size_t(-1).value)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_smooth_bodies_jvp_(out, *args, **td, tangents=V, algo="chunked")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_smooth_bodies_jvp_(out, *args, **td, tangents=V, algo="ordered")
    with pytest.raises(ValueError):  # a workspace shorter than the queried size
        short = torch.empty(need - 256, dtype=torch.uint8, device=dev)
        dpr_amd.raster_smooth_bodies_jvp_(out, *args, **td, tangents=V, algo="tiled", workspace=short)
    with pytest.raises(dpr_amd.DprError):  # V = 17
        dpr_amd.raster_smooth_bodies_jvp_(out, *args, **td, tangents=17)
    with pytest.raises(dpr_amd.DimensionMismatch):  # rotation_dot without its K axis
        dpr_amd.raster_smooth_bodies_jvp_(out, *args, rotation_dot=td["rotation_dot"][:, :, 0], tangents=V)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the same through the C entry point, which reports a status and launches nothing
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    pts, body, rot, trans, _bg, ow, pw = args
    body32 = body.to(torch.int32)
    rot_cm = rot.transpose(-1, -2).contiguous()
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(algo=_lib.ALGO_ATOMIC, flags=0, ni=n_in, no=n_out, k=K, v=V, wsb=0):
        return L.dpr_raster_smooth_bodies_jvp_ex_f32(
            st, algo, flags, ni, no, gp, P, B, k, v, ptr(out), ptr(pts), ptr(body32), ptr(rot_cm), ptr(trans), ptr(ow),
            ptr(pw), ptr(td["points_dot"]), None, None, None, None, None, ptr(ws) if wsb else None, wsb)

    assert call(v=17) == _lib.ERR_INVALID_ARG and call(v=0) == _lib.ERR_INVALID_ARG
    assert call(k=0) == _lib.ERR_INVALID_ARG
    assert call(ni=2, no=3) == _lib.ERR_UNSUPPORTED_DIMS
    assert call(algo=_lib.ALGO_CHUNKED) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(flags=_lib.FLAG_KEEP_BINNING) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(algo=_lib.ALGO_TILED) == _lib.ERR_WORKSPACE
    assert call(algo=_lib.ALGO_TILED, wsb=need - 256) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(algo=_lib.ALGO_TILED, wsb=need) == _lib.OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
