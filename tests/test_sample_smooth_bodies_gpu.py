"""Smooth sampling at the points of rigid bodies on the GPU (dpr_amd.sample_smooth_bodies / sample_smooth_bodies_ /
sample_smooth_bodies_pullback_ / sample_smooth_bodies_ad; include/dpr.h, SMOOTH SAMPLING, RIGID BODIES; kernels:
csrc/dpr_sample_smooth_bodies.hip) against tests/sample_smooth_bodies_reference.py, the numpy smooth-sampling reference
composed per body and evaluated in fp64.  Tolerances: tol(npdt, kind) of tests/test_parity_gpu.py (fp64 1e-10; fp32 5e-5
ds_dimage, 1e-4 values and ds_dpoints, 1e-3 pose gradients), norm-wise, the pose gradients per (image, body).

Shapes: those of tests/test_smooth_bodies_gpu.py, whose `_case` draws the clouds (and asserts, there, that they reach
their hazards): grids (70, 19), (18, 9, 10) and (5, 7), P = 777, B = 3, K = 3, sorted and shuffled; the image is that
case's `g`, ds_dvalues is drawn here."""
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import sample_smooth_bodies_reference as ref
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol
from tests.test_smooth_bodies_gpu import GRIDS, MIX, SMALL, _accepted, _case
from tests.test_smooth_clouds_gpu import _cloud, _coords, _poses

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
BWD = ("atomic", "tiled", "auto")
NAMES = ("image", "points", "rotation", "translation")
KINDS = ("out", "points", "pose", "pose")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _scase(n_in, n_out, grid=None, sizes=(259, 259, 259), B=3, order="sorted", seed=0, labels=0):
    """The inputs of `_case` (its ds_dout is the image here), ds_dvalues, and the fp64 reference results, computed once
    and shared; never modified.  labels > 0: `body` remapped onto that many labels, body + len(sizes) * (i % m) for
    point i, every label with the pose of the body it came from."""
    c = _case(n_in, n_out, grid=grid, sizes=sizes, B=B, order=order, seed=seed)
    body, rot, trans, K = np.array(c["body"]), c["rot"], c["trans"], c["K"]
    if labels:
        m = labels // K
        body = body + K * (np.arange(c["P"]) % m)
        src = np.arange(labels) % K
        rot, trans, K = np.ascontiguousarray(rot[:, src]), np.ascontiguousarray(trans[:, src]), labels
        assert body.max() < K and len(np.unique(body)) > 32
    dv = np.random.default_rng(900 + seed).normal(size=(c["P"], B))
    s = dict(grid=c["grid"], points=c["points"], body=body, rot=rot, trans=trans, image=c["g"], dv=dv, B=B, K=K,
             P=c["P"], base=c)
    s["values"] = ref.sample(s["image"], s["points"], body, rot, trans)
    s["pb"] = ref.sample_pullback(dv, s["image"], s["points"], body, rot, trans)
    return _freeze(s)


def _args(s, dev, npdt, body_dtype=torch.int64):
    """(image, points, body, rotation, translation) on the device"""
    f = lambda k: T(s[k].astype(npdt), dev)
    return [grid_to_dev(s["image"].astype(npdt), dev), f("points"),
            torch.as_tensor(np.array(s["body"]), device=dev).to(body_dtype), f("rot"), f("trans")]


def _dv(s, dev, npdt):
    """ds_dvalues (P, B) with the point index fastest"""
    return T(np.ascontiguousarray(s["dv"].T).astype(npdt), dev).t()


def _check_pullback(pb, want, npdt, what=""):
    for name, kind, a, e in zip(NAMES, KINDS, pb, want):
        if a is None:
            continue
        if name in ("rotation", "translation"):  # per (image, body): the norm of one body does not hide another's
            assert tuple(a.shape) == e.shape, name
            for b in range(e.shape[0]):
                for k in range(e.shape[1]):
                    assert_close(a[b, k], e[b, k].astype(npdt), tol(npdt, kind), f"{what}ds_d{name}[{b}, {k}]")
        elif name == "image":
            for b in range(e.shape[-1]):
                assert_close(a[..., b], e[..., b].astype(npdt), tol(npdt, kind), f"{what}ds_dimage plane {b}")
        else:
            assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}ds_d{name}")


def _grids(n_out):
    return [GRIDS[n_out]] + ([SMALL] if n_out == 2 else [])


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("body_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_forward_and_pullback_match_the_reference(dev, body_dtype, order, npdt, tdt, n_in, n_out):
    for grid in _grids(n_out):
        s = _scase(n_in, n_out, grid=grid, order=order)
        assert s["P"] == 777 and s["B"] == 3 and s["K"] == 3
        assert (np.diff(s["body"]) >= 0).all() == (order == "sorted")
        acc = _accepted(s["base"])
        assert (acc.any(axis=0) & ~acc.all(axis=0)).any()  # rejected in one image, accepted in another
        args = _args(s, dev, npdt, body_dtype)
        for algo in ("atomic", "auto"):
            values = dpr_amd.sample_smooth_bodies(*args, algo=algo)
            assert values.shape == (777, 3) and values.dtype == tdt and values.t().is_contiguous()
            assert_close(values, s["values"].astype(npdt), tol(npdt, "points"), f"{grid} {algo} values")
            assert bool((values.t()[torch.as_tensor(~acc, device=dev)] == 0).all())
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.sample_smooth_bodies(*args, algo="tiled")
        dv = _dv(s, dev, npdt)
        never = torch.as_tensor(np.flatnonzero(~acc.any(axis=0)), device=dev)
        assert len(never) > 0
        for algo in BWD:
            pb = dpr_amd.sample_smooth_bodies_pullback_(dv, *args, algo=algo)
            assert pb.image.shape == grid + (3,) and pb.points.shape == (777, n_in)
            assert pb.rotation.shape == (3, 3, n_out, n_in) and pb.translation.shape == (3, 3, n_out)
            _check_pullback(pb, s["pb"], npdt, f"{grid} {algo} ")
            assert bool((pb.points[never] == 0).all())
        assert dpr_amd.resolve_algo_sample_smooth_bodies("pullback", grid, 777, 3, 3, n_in) == "atomic"


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_values_do_not_depend_on_the_order_of_the_cloud(dev, npdt, tdt, n_in, n_out):
    """The forward has no sum across threads: scalar pose loads (a wave of one body) and per-lane gathers (a mixed
    wave) give the same bits.  The shuffled case is the sorted cloud under a permutation."""
    a, b = _scase(n_in, n_out, order="sorted"), _scase(n_in, n_out, order="shuffled")
    perm = np.random.default_rng(7).permutation(a["P"])  # (that of tests/test_smooth_bodies_gpu.py::_case)
    assert np.array_equal(a["points"][perm], b["points"]) and np.array_equal(a["body"][perm], b["body"])
    va = dpr_amd.sample_smooth_bodies(*_args(a, dev, npdt))
    vb = dpr_amd.sample_smooth_bodies(*_args(b, dev, npdt))
    assert float(va.abs().max()) > 0
    assert torch.equal(va[torch.as_tensor(perm, device=dev)], vb)


# ------------------------------------------------------------------ 2. composition of the single-body operator
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_one_body_is_sample_smooth(dev, npdt, tdt, n_in, n_out):
    s = _scase(n_in, n_out, sizes=(777,), seed=1)
    img, pts, body, rot, trans = _args(s, dev, npdt)
    dv = _dv(s, dev, npdt)
    values = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    assert torch.equal(values, dpr_amd.sample_smooth(img, pts, rot[:, 0], trans[:, 0]))
    assert_close(values, s["values"].astype(npdt), tol(npdt, "points"), "values against the reference")
    want = dpr_amd.sample_smooth_pullback_(dv, img, pts, rot[:, 0], trans[:, 0], algo="atomic")
    for algo in BWD:
        pb = dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, rot, trans, algo=algo)
        assert_close(pb.image, want.image.cpu().numpy(), tol(npdt, "out"), f"{algo} ds_dimage")
        assert_close(pb.points, want.points.cpu().numpy(), tol(npdt, "points"), f"{algo} ds_dpoints")
        for b in range(3):
            assert_close(pb.rotation[b, 0], want.rotation[b].cpu().numpy(), tol(npdt, "pose"), f"{algo} dR[{b}]")
            assert_close(pb.translation[b, 0], want.translation[b].cpu().numpy(), tol(npdt, "pose"), f"{algo} dt[{b}]")
    # one image: one thread adds one pose's terms in k_sample_smooth_bwd's order and stores them
    p1 = dpr_amd.sample_smooth_pullback_(dv[:, 0], img[..., 0].contiguous(), pts, rot[0, 0], trans[0, 0],
                                         need=("points",), algo="atomic")
    pb = dpr_amd.sample_smooth_bodies_pullback_(dv[:, 0], img[..., 0].contiguous(), pts, body, rot[0], trans[0],
                                                need=("points",), algo="atomic")
    assert float(p1.points.abs().max()) > 0 and torch.equal(pb.points, p1.points)


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_every_piece_is_that_of_the_subset_calls(dev, npdt, tdt, n_in, n_out):
    s = _scase(n_in, n_out, order="shuffled")
    img, pts, body, rot, trans = _args(s, dev, npdt)
    dv = _dv(s, dev, npdt)
    values = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    pbs = {a: dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, rot, trans, algo=a) for a in ("atomic", "tiled")}
    total = torch.zeros_like(pbs["atomic"].image)
    for k in range(s["K"]):
        idx = torch.nonzero(body == k).flatten()
        sub = (img, pts[idx].contiguous(), rot[:, k].contiguous(), trans[:, k].contiguous())
        assert torch.equal(values[idx], dpr_amd.sample_smooth(*sub))
        dvk = dv[idx].t().contiguous().t()
        p1 = dpr_amd.sample_smooth_pullback_(dvk, *sub, algo="atomic")
        total += p1.image
        for a, pb in pbs.items():
            assert_close(pb.points[idx], p1.points.cpu().numpy(), tol(npdt, "points"), f"{a} ds_dpoints of body {k}")
            for b in range(s["B"]):
                assert_close(pb.rotation[b, k], p1.rotation[b].cpu().numpy(), tol(npdt, "pose"), f"{a} dR[{b}, {k}]")
                assert_close(pb.translation[b, k], p1.translation[b].cpu().numpy(), tol(npdt, "pose"),
                             f"{a} dt[{b}, {k}]")
    for a, pb in pbs.items():
        for b in range(s["B"]):
            assert_close(pb.image[..., b], total[..., b].cpu().numpy(), tol(npdt, "out"), f"{a} ds_dimage plane {b}")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_image_gradient_is_the_splat_and_the_adjoint_identity_holds(dev, npdt, tdt, n_in, n_out):
    """ds_dimage[.., b] on TILED against raster_smooth_bodies_(algo="tiled") of image b with weights ds_dvalues[:, b];
    and sum_v raster_smooth_bodies(pw)[v, b] * image[v, b] = sum_p pw[p] * values[p, b] on the device, to tol relative
    to the sum of the magnitudes of the terms."""
    s = _scase(n_in, n_out, order="shuffled")
    img, pts, body, rot, trans = _args(s, dev, npdt)
    dv = _dv(s, dev, npdt)
    d_img = dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, rot, trans, need=("image",), algo="tiled").image
    for b in range(3):
        want = dpr_amd.raster_smooth_bodies(s["grid"], pts, body, rot[b], trans[b], None, None, dv[:, b].contiguous(),
                                            algo="tiled")
        assert_close(d_img[..., b], want.cpu().numpy(), tol(npdt, "out"), f"plane {b}")
    pw = T(np.random.default_rng(3).uniform(0.5, 1.5, size=s["P"]).astype(npdt), dev)
    out = dpr_amd.raster_smooth_bodies(s["grid"], pts, body, rot, trans, None, None, pw, algo="atomic")
    values = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    for b in range(3):
        lhs = float((out[..., b].double() * img[..., b].double()).sum())
        terms = pw.double() * values[:, b].double()
        assert abs(lhs - float(terms.sum())) <= tol(npdt, "points") * float(terms.abs().sum()), b


# ------------------------------------------------------------------ 3. dropped points, empty bodies
@pytest.mark.parametrize("body_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_bodies_out_of_range_are_dropped(dev, body_dtype, npdt, tdt, n_in, n_out):
    """-1, K and 2^31 - 1 (int64: also +-2^40, clamped by the wrapper): exact zeros in values and ds_dpoints, nothing in
    ds_dimage or the pose gradients -- the results of the call without them."""
    s = _scase(n_in, n_out, order="shuffled")
    K = s["K"]
    bad = np.arange(100, 130)  # (the cloud is shuffled: points of every body)
    body = np.array(s["body"])
    body[bad] = np.resize([-1, K, 2**31 - 1], 30)
    if body_dtype == torch.int64:
        body[bad[:4]] = (2**40, -(2**40), 2**40 + 1, -(2**40) + 2)
    keep = np.setdiff1d(np.arange(s["P"]), bad)
    img, pts, _, rot, trans = _args(s, dev, npdt)
    tb = torch.as_tensor(body, device=dev).to(body_dtype)
    dv = _dv(s, dev, npdt)
    values = dpr_amd.sample_smooth_bodies(img, pts, tb, rot, trans)
    assert bool((values[bad] == 0).all())
    assert torch.equal(values[keep], dpr_amd.sample_smooth_bodies(img, pts[keep].contiguous(), tb[keep].contiguous(),
                                                                  rot, trans))
    want = ref.sample_pullback(s["dv"][keep], s["image"], s["points"][keep], body[keep], s["rot"], s["trans"])
    for algo in ("atomic", "tiled"):
        pb = dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, tb, rot, trans, algo=algo)
        assert bool((pb.points[bad] == 0).all())
        _check_pullback((pb.image, pb.points[keep], pb.rotation, pb.translation), want, npdt, f"{algo} ")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_a_body_without_points_gets_exact_zeros(dev, npdt, tdt, n_in, n_out):
    s = _scase(n_in, n_out, sizes=(300, 200, 0, 277), seed=2)
    assert s["K"] == 4 and 2 not in s["body"]
    args = _args(s, dev, npdt)
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=tdt, device=dev)
    d_rot, d_trans = nan(3, 4, n_in, n_out).transpose(-1, -2), nan(3, 4, n_out)
    pb = dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *args, ds_drotation=d_rot, ds_dtranslation=d_trans)
    assert pb.translation is d_trans and pb.rotation.data_ptr() == d_rot.data_ptr()
    assert bool((pb.rotation[:, 2] == 0).all()) and bool((pb.translation[:, 2] == 0).all())
    _check_pullback(pb, s["pb"], npdt)


# ------------------------------------------------------------------ 4. the per-(image, body) sums
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_wave_and_block_mixes(dev, B, order, npdt, tdt, n_in, n_out):
    """P = 640 sorted with body sizes 256, 64, 64, 100, 156: block 0 holds one body (wave -> block -> one atomic);
    block 1 holds waves of one body each in a mixed block (bodies 1, 2) and mixed waves (3 into 4), block 2 is a partial
    block: both on the LDS table (K = 5).  Shuffled: every wave walks five bodies into the table.  B = 1: plain stores
    of the point gradients; B = 3: three slices, atomics onto zeroed buffers."""
    s = _scase(n_in, n_out, sizes=MIX, B=B, order=order, seed=3)
    if order == "sorted":
        per_wave = [len(np.unique(s["body"][i:i + 64])) for i in range(0, 640, 64)]
        assert len(np.unique(s["body"][:256])) == 1 and per_wave[4] == 1 and per_wave[5] == 1 and 2 in per_wave[6:]
    else:
        assert min(len(np.unique(s["body"][i:i + 64])) for i in range(0, 640, 64)) == 5
    args = _args(s, dev, npdt)
    nan = torch.full((640, n_in), float("nan"), dtype=tdt, device=dev)
    pb = dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *args, ds_dpoints=nan, algo="atomic")
    assert pb.points is nan
    _check_pullback(pb, s["pb"], npdt, f"{order} B={B} ")
    assert_close(dpr_amd.sample_smooth_bodies(*args), s["values"].astype(npdt), tol(npdt, "points"), "values")


@pytest.mark.parametrize("labels", [64, 65, 200])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_many_bodies_in_a_block(dev, labels, npdt, tdt, n_in, n_out):
    """The same cloud, shuffled, with `body` remapped onto K = 64 labels (the largest LDS table), 65 and 200 (the walk
    with global atomics)."""
    if labels == 64:
        s = _scase(n_in, n_out, sizes=(10,) * 64, order="shuffled", seed=6)
        assert s["K"] == 64 and max(len(np.unique(s["body"][i:i + 256])) for i in range(0, 640, 256)) > 32
    else:
        s = _scase(n_in, n_out, sizes=MIX, order="shuffled", seed=3, labels=labels)
        assert s["K"] == labels and s["P"] == 640
    pb = dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *_args(s, dev, npdt), algo="atomic")
    assert pb.rotation.shape == (3, s["K"], n_out, n_in)
    _check_pullback(pb, s["pb"], npdt, f"K={labels} ")
    empty = np.setdiff1d(np.arange(s["K"]), s["body"])
    assert bool((pb.rotation[:, empty] == 0).all()) and bool((pb.translation[:, empty] == 0).all())


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_many_slices_of_images(dev, n_in, n_out):
    """B = 70, P = 300: two blocks of points, so every image is a slice of its own."""
    s = _scase(n_in, n_out, sizes=(100, 100, 100), B=70, order="shuffled", seed=7)
    args = _args(s, dev, np.float64)
    assert_close(dpr_amd.sample_smooth_bodies(*args), s["values"], 1e-10, "values")
    _check_pullback(dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, np.float64), *args), s["pb"], np.float64)


def test_one_slice_for_several_images_stores_the_point_gradients(dev):
    """P = 524 288 + 5 (2049 blocks), B = 2, K = 4, fp32: pose_slices gives one slice, so ds_dpoints of several images
    is summed in registers and stored; every smaller batch adds it atomically.  Against the loop of K subset calls of
    sample_smooth / sample_smooth_pullback_ on the device."""
    n_in, n_out, grid, P, B, K = 3, 2, GRIDS[2], 524288 + 5, 2, 4
    g = torch.Generator(device="cpu").manual_seed(5)
    pts = (torch.rand(P, n_in, generator=g) * 2.2 - 1.1).to(dev)
    body = torch.randint(0, K, (P,), generator=g).to(dev)
    q, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(B * K, n_in, n_in)))
    rot = T(q[:, :n_out].reshape(B, K, n_out, n_in).astype(np.float32), dev)
    trans = (torch.rand(B, K, n_out, generator=g) * 0.2 - 0.1).to(dev)
    img = dpr_amd.to_grid_layout(torch.randn(grid + (B,), generator=g).to(dev))
    dv = torch.randn(B, P, generator=g).to(dev).t()
    values = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    nan = torch.full((P, n_in), float("nan"), device=dev)
    pb = dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, rot, trans, ds_dpoints=nan, algo="atomic")
    total = torch.zeros_like(pb.image)
    for k in range(K):
        idx = torch.nonzero(body == k).flatten()
        sub = (img, pts[idx].contiguous(), rot[:, k].contiguous(), trans[:, k].contiguous())
        assert torch.equal(values[idx], dpr_amd.sample_smooth(*sub))
        p1 = dpr_amd.sample_smooth_pullback_(dv[idx].t().contiguous().t(), *sub, algo="atomic")
        total += p1.image
        assert_close(pb.points[idx], p1.points.cpu().numpy(), 1e-4, f"ds_dpoints of body {k}")
        for b in range(B):
            assert_close(pb.rotation[b, k], p1.rotation[b].cpu().numpy(), 1e-3, f"dR[{b}, {k}]")
            assert_close(pb.translation[b, k], p1.translation[b].cpu().numpy(), 1e-3, f"dt[{b}, {k}]")
    for b in range(B):
        assert_close(pb.image[..., b], total[..., b].cpu().numpy(), 5e-5, f"ds_dimage plane {b}")


# ------------------------------------------------------------------ 5. groups of images, subsets of the outputs
@pytest.mark.parametrize("group", [1, 2, 0])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_groups_of_images(dev, group, npdt, tdt, n_in, n_out):
    """B = 5: max_pose_group 1 (image by image), 2 (groups of 2 + 2 + 1) and 0 (all five images in one group)."""
    s = _scase(n_in, n_out, sizes=(100, 100, 100), B=5, order="shuffled", seed=4)
    args = _args(s, dev, npdt)
    buf = dpr_amd.empty_grid(s["grid"], 5, tdt, dev).fill_(float("nan"))
    pb = dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *args, ds_dimage=buf, algo="tiled",
                                                max_pose_group=group)
    assert pb.image is buf and bool(torch.isfinite(buf).all())
    _check_pullback(pb, s["pb"], npdt, f"group {group} ")
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *args, algo="tiled", max_pose_group=17)
    with pytest.raises(dpr_amd.DprError):  # (no groups anywhere but on the TILED pullback)
        dpr_amd.sample_smooth_bodies_pullback_(_dv(s, dev, npdt), *args, algo="atomic", max_pose_group=2)


@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_need_subsets_write_only_their_buffers(dev, algo, npdt, tdt, n_in, n_out):
    s = _scase(n_in, n_out, order="shuffled")
    img, pts, body, rot, trans = _args(s, dev, npdt)
    dv = _dv(s, dev, npdt)
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=tdt, device=dev)
    for need in (("image",), ("points",), ("rotation",), ("translation",), ("points", "translation"),
                 ("image", "rotation")):
        bufs = dict(image=dpr_amd.empty_grid(s["grid"], 3, tdt, dev).fill_(float("nan")), points=nan(777, n_in),
                    rotation=nan(3, 3, n_in, n_out).transpose(-1, -2), translation=nan(3, 3, n_out))
        kw = {f"ds_d{n}": bufs[n] for n in need}
        pb = dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, rot, trans, need=need, algo=algo, **kw)
        for n, got in zip(NAMES, pb):
            if n in need:
                assert got.data_ptr() == bufs[n].data_ptr() and bool(torch.isfinite(got).all()), (need, n)
            else:
                assert got is None and bool(torch.isnan(bufs[n]).all()), (need, n)
        _check_pullback(pb, s["pb"], npdt, f"{algo} need={need} ")
    # ds_dimage does not read the image
    pb = dpr_amd.sample_smooth_bodies_pullback_(dv, None, pts, body, rot, trans, need=("image",), algo=algo,
                                                grid_size=s["grid"])
    _check_pullback(pb, s["pb"], npdt, f"{algo} image=None ")
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_bodies_pullback_(dv, None, pts, body, rot, trans, need=("image", "points"),
                                               grid_size=s["grid"])


# ------------------------------------------------------------------ 6. edge shapes
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_no_points_one_point_no_images_a_nan_point_and_the_single_image_form(dev, algo, npdt, tdt, n_in, n_out):
    s = _scase(n_in, n_out)
    grid, B, K, P = s["grid"], s["B"], s["K"], s["P"]
    img, pts, body, rot, trans = _args(s, dev, npdt)
    dv = _dv(s, dev, npdt)
    # P = 0
    assert dpr_amd.sample_smooth_bodies(img, pts[:0], body[:0], rot, trans).shape == (0, B)
    pb = dpr_amd.sample_smooth_bodies_pullback_(dv[:0], img, pts[:0], body[:0], rot, trans, algo=algo)
    assert pb.points.shape == (0, n_in)
    assert bool((pb.image == 0).all()) and bool((pb.rotation == 0).all()) and bool((pb.translation == 0).all())
    # P = 1 (an accepted point of body 1)
    i = int(np.flatnonzero((s["body"] == 1) & _accepted(s["base"]).all(axis=0))[0])
    sl = slice(i, i + 1)
    one = (img, pts[sl].contiguous(), body[sl].contiguous(), rot, trans)
    assert_close(dpr_amd.sample_smooth_bodies(*one), s["values"][sl].astype(npdt), tol(npdt, "points"), "P=1")
    want = ref.sample_pullback(s["dv"][sl], s["image"], s["points"][sl], s["body"][sl], s["rot"], s["trans"])
    pb1 = dpr_amd.sample_smooth_bodies_pullback_(dv[sl], *one, algo=algo)
    _check_pullback(pb1, want, npdt, "P=1 ")
    assert bool((pb1.rotation[:, [0, 2]] == 0).all())
    # B = 0: empty values, images and pose gradients, zero point gradients
    e = lambda *sh: torch.zeros(sh, dtype=tdt, device=dev)
    none = (dpr_amd.empty_grid(grid, 0, tdt, dev), pts, body, e(0, K, n_out, n_in), e(0, K, n_out))
    assert dpr_amd.sample_smooth_bodies(*none).shape == (P, 0)
    nan = torch.full((P, n_in), float("nan"), dtype=tdt, device=dev)
    pb = dpr_amd.sample_smooth_bodies_pullback_(e(0, P).t(), *none, ds_dpoints=nan, algo=algo)
    assert pb.rotation.shape == (0, K, n_out, n_in) and pb.image.shape == grid + (0,) and bool((pb.points == 0).all())
    # a NaN point: rejected, 0 everywhere, and the other points as before
    bad = pts.clone()
    bad[5] = float("nan")
    values = dpr_amd.sample_smooth_bodies(img, bad, body, rot, trans)
    ok = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    assert bool((values[5] == 0).all()) and torch.equal(values[6:], ok[6:]) and torch.equal(values[:5], ok[:5])
    pbn = dpr_amd.sample_smooth_bodies_pullback_(dv, img, bad, body, rot, trans, algo=algo)
    assert bool((pbn.points[5] == 0).all()) and all(bool(torch.isfinite(t).all()) for t in pbn)
    # the single-image form: no B axis anywhere
    b = 1
    v1 = dpr_amd.sample_smooth_bodies(img[..., b].contiguous(), pts, body, rot[b], trans[b])
    assert v1.shape == (P,)
    assert_close(v1, s["values"][:, b].astype(npdt), tol(npdt, "points"), "single image")
    s1 = dpr_amd.sample_smooth_bodies_pullback_(dv[:, b].contiguous(), img[..., b].contiguous(), pts, body, rot[b],
                                                trans[b], algo=algo)
    assert s1.image.shape == grid and s1.rotation.shape == (K, n_out, n_in) and s1.translation.shape == (K, n_out)
    want1 = ref.sample_pullback(s["dv"][:, b:b + 1], s["image"][..., b:b + 1], s["points"], s["body"],
                                s["rot"][b:b + 1], s["trans"][b:b + 1])
    _check_pullback((s1.image[..., None], s1.points, s1.rotation[None], s1.translation[None]), want1, npdt,
                    "single image ")


# ------------------------------------------------------------------ 7. the exact derivative, fp64
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_agrees_with_central_differences(dev, algo, n_in, n_out):
    """sample_smooth_bodies_ad in fp64 on an 8^N grid with 2 images, 3 bodies and 12 points: central differences with
    h = 1e-6 of sum(values * dv) in image, points, rotation and translation, within 1e-6 * max|gradient|."""
    rng = np.random.default_rng(11)
    nb, K, npts, grid = 2, 3, 12, (8,) * n_out
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(npts, n_in)), rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out)]
    body = torch.as_tensor(np.arange(npts) % K, device=dev)
    dv = T(rng.normal(size=(nb, npts)), dev).t()
    image = grid_to_dev(rng.normal(size=grid + (nb,)), dev).requires_grad_(True)
    xs = [image] + [torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in vals]
    values = dpr_amd.sample_smooth_bodies_ad(xs[0], xs[1], body, xs[2], xs[3], algo=algo)
    (values * dv).sum().backward()
    grads = [x.grad.cpu().numpy() for x in xs]
    scale = max(np.abs(a).max() for a in grads)
    h = 1e-6
    with torch.no_grad():
        loss = lambda: float((dpr_amd.sample_smooth_bodies(xs[0], xs[1], body, xs[2], xs[3]) * dv).sum())
        for name, x, ga in zip(NAMES, xs, grads):
            fd = np.zeros(ga.shape)
            for i in np.ndindex(*ga.shape):
                keep = float(x[i])
                x[i] = keep + h
                up = loss()
                x[i] = keep - h
                dn = loss()
                x[i] = keep
                fd[i] = (up - dn) / (2 * h)
            err = np.abs(fd - ga).max()
            assert err <= 1e-6 * scale, (name, err, scale)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_values_and_gradients_are_continuous_across_a_cell_face(dev, n_in, n_out):
    """Every point of body 1 sits 1e-9 cells either side of a cell face of axis 0 in image 1 (fp64): the values and the
    gradients of the two calls differ by less than 1e-6 * their largest entry."""
    rng = np.random.default_rng(5)
    grid, nb, K, per = (8,) * n_out, 3, 3, 6
    image = grid_to_dev(rng.normal(size=grid + (nb,)), dev)
    rot, trans = _poses(rng, nb * K, n_in, n_out)
    rot, trans = rot.reshape(nb, K, n_out, n_in), trans.reshape(nb, K, n_out)
    pts = np.concatenate([_cloud(rng, grid, rot[1, k], trans[1, k], n_in, per, lo=1.0, hi=-1.0) for k in range(K)])
    body = np.repeat(np.arange(K), per)
    dv = T(rng.normal(size=(nb, K * per)), dev).t()
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
    common = (tb, T(rot, dev), T(trans, dev))
    va, vb = (dpr_amd.sample_smooth_bodies(image, T(p, dev), *common) for p in (lo, hi))
    assert float((va - vb).abs().max()) < 1e-6 * float(va.abs().max())
    pa, pb = (dpr_amd.sample_smooth_bodies_pullback_(dv, image, T(p, dev), *common) for p in (lo, hi))
    scale = max(float(a.abs().max()) for a in pa)
    for a, b in zip(pa, pb):
        assert float((a - b).abs().max()) < 1e-6 * scale
