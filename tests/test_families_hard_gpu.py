"""The TILED channel, JVP, sampling and per-pose-cloud paths -- and the pose slices of the direct kernels -- on the
inputs where a binned kernel goes wrong: grids of several tiles with remainders on every axis, tiles split into
parts and recombined from overflow slabs next to tiles that are split too, a Morton-sorted cloud (the blocked
record assignment), points on cell faces, outside the grid and with NaN / Inf coordinates.

Every expectation is the CPU oracle (tests/test_jvp_abi.py's restatement for the JVP).  All inputs are rounded to
fp32 once and used for both dtypes, so `ref64` -- the fp64 oracle on these inputs -- is the fp64 tests' reference
and the truth behind the fp32 tests' element-wise check.

Tiles (3-D 64 x 16 x 8, 2-D 32 x 32) and records per tile, counted on the CPU from the oracle's cell choice
(`tile_counts`; a point is a record of the tile that holds max(ref0, 0)); "split" is more than SPLIT records
(3-D 8192, 2-D 2048: split on every path), "pairs" counts face-adjacent split tiles, ">4096" the tiles above 4096 records:

    input          grid            tiles      pose 0: split (pairs), >4096 (pairs)   pose 1                pose 2
    H3             (130, 70, 37)   3 x 5 x 5  2 (1), 4 (4)                           2 (1), 2 (1)          2 (1), 2 (1)
    H2_22, H2_32   (100, 70)       4 x 3      2 (1), 1 (0)                           2 (1), 2 (1)          2 (1) / 3 (2), 2 (1)
    S3             (96, 40, 24)    2 x 3 x 3  2 (1), 4 (3)                           2 (1), 4 (3)          2 (1), 5 (4)
    clouds         (130, 70, 37)   3 x 5 x 5  cloud 0: 2 (1), heaviest tile 20168    cloud 1: none, 3445   cloud 2: 2 (1), 12928

(The heaviest tiles of H3, H2 and S3 hold 73 000 - 116 000, 21 000 - 37 000 and 14 000 - 19 000 records.)

The fp32 element-wise bound  max|got - ref64| <= m * max|ref64|  per plane: `rho` is the reference's own rounding at
this input, max over planes of max|ref32 - ref64| / max|ref64| with ref32 the fp32 oracle (for out_dot: the
restatement with value_dtype = fp32), measured on the CPU; m = 4 rho (the device sums in another order but in
at least the oracle's precision).  No cell is skipped.

    family / input            rho          m
    channels / H3             4.693e-06    1.877e-05
    channels / H2_22          3.179e-06    1.272e-05
    channels / H2_32          2.732e-06    1.093e-05
    channels / S3             3.341e-06    1.336e-05
    sample / H3               7.489e-06    2.996e-05
    sample / H2_22            7.323e-06    2.929e-05
    sample / H2_32            1.090e-05    4.360e-05
    clouds / H3               3.454e-06    1.382e-05
    jvp_all / H3              7.018e-06    2.807e-05
    jvp_point_weight / H3     3.002e-06    1.201e-05
    jvp_all / H2_22           6.493e-06    2.597e-05
    jvp_point_weight / H2_22  1.732e-06    6.928e-06
    jvp_all / H2_32           5.545e-06    2.218e-05
    jvp_point_weight / H2_32  1.121e-06    4.484e-06
    jvp_all / S3              2.812e-07    1.125e-06
    jvp_point_weight / S3     2.488e-07    9.952e-07
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from oracle import oracle
from tests import data as D
from tests.test_channels_gpu import _bit_equal_or_rounding, assert_close, oracle_plane, plane, tol
from tests.test_clouds_gpu import check_against_oracle, on as clouds_on
from tests.test_jvp_abi import KINDS, jvp_reference, random_tangents
from tests.test_jvp_gpu import tol as jvp_tol

pytestmark = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
TILE = {3: (64, 16, 8), 2: (32, 32)}
# A tile is split into parts above max(P / 256, 4096) records (3-D; twice that in a forward-only call) or above
# max(P / 2048, 2048) records (2-D) -- make_plan in csrc/dpr_tiled_plan.hip.  Above SPLIT records a tile of these inputs
# is split on every path.
SPLIT = {3: 8192, 2: 2048}
SPEC = {  # name: n_in, n_out, grid, points, kind, seed
    "H3": (3, 3, (130, 70, 37), 150_000, "cluster", 27),
    "H2_22": (2, 2, (100, 70), 40_000, "cluster", 42),
    "H2_32": (3, 2, (100, 70), 40_000, "cluster", 42),
    "S3": (3, 3, (96, 40, 24), 60_000, "morton", 23),
}
INPUTS = tuple(SPEC)
# rho of the module docstring; the bound is M_FACTOR * rho
M_FACTOR = 4.0
RHO = {
    ("channels", "H3"): 4.693e-06,
    ("channels", "H2_22"): 3.179e-06,
    ("channels", "H2_32"): 2.732e-06,
    ("channels", "S3"): 3.341e-06,
    ("sample", "H3"): 7.489e-06,
    ("sample", "H2_22"): 7.323e-06,
    ("sample", "H2_32"): 1.090e-05,
    ("clouds", "H3"): 3.454e-06,
    ("jvp_all", "H3"): 7.018e-06,
    ("jvp_point_weight", "H3"): 3.002e-06,
    ("jvp_all", "H2_22"): 6.493e-06,
    ("jvp_point_weight", "H2_22"): 1.732e-06,
    ("jvp_all", "H2_32"): 5.545e-06,
    ("jvp_point_weight", "H2_32"): 1.121e-06,
    ("jvp_all", "S3"): 2.812e-07,
    ("jvp_point_weight", "S3"): 2.488e-07,
}


def r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def to(a, tdt, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)


# ------------------------------------------------------------------ the hard inputs
def face_and_bad_points(rng, n_in, n_out, grid):
    """F: 64 points whose leading coordinates are cell faces -1 + 2 k / n (k = 0 and k = n among them) under the
    identity pose, and 5 points with NaN / Inf coordinates."""
    faces = 0.3 * rng.normal(size=(64, n_in))
    for j in range(min(n_in, n_out)):
        k = rng.integers(0, grid[j] + 1, size=64)
        k[0], k[1] = 0, grid[j]
        k[2], k[3] = (0, grid[j]) if j == 0 else (grid[j], 0)
        faces[:, j] = -1.0 + 2.0 * k / grid[j]
    bad = np.full((5, n_in), 0.1)
    bad[0, 0] = np.nan
    bad[1, -1] = np.inf
    bad[2, 0] = -np.inf
    bad[3, :] = np.nan
    bad[4, 0], bad[4, -1] = np.inf, np.nan
    return np.concatenate([faces, bad])


@functools.lru_cache(maxsize=None)
def hard(name):
    n_in, n_out, grid, P, kind, seed = SPEC[name]
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=3, grid_n=grid, seed=seed)
    pts = d.points.copy()
    if kind == "cluster":  # the recipe of test_heavy_tiles_are_split
        pts *= 0.12
        pts[::50] *= 8.0
    else:  # Morton order, as in test_chunked_on_spatially_sorted_points
        q = np.clip(((pts * 0.5 + 0.5) * 1024).astype(np.int64), 0, 1023)
        code = np.zeros(len(q), dtype=np.int64)
        for bit in range(10):
            for k in range(n_in):
                code |= ((q[:, k] >> bit) & 1) << (n_in * bit + k)
        pts = pts[np.argsort(code, kind="stable")]
    rot, trans = d.rotations.copy(), d.translations.copy()
    rot[0] = np.eye(n_out, n_in)
    trans[0] = 0.0
    pts = np.concatenate([pts, face_and_bad_points(np.random.default_rng(seed + 1000), n_in, n_out, grid)])
    return SimpleNamespace(name=name, n_in=n_in, n_out=n_out, grid=grid, P=len(pts), B=3, points=r32(pts),
                           rot=r32(rot), trans=r32(trans))


def tile_counts(grid, points, rot, trans):
    """Records per tile of one pose, from the oracle's cell choice: ref0 = ceil(coord - 0.5) - 1 of the points with
    -1 < coord - 0.5 <= n on every axis; the tile is the one that holds max(ref0, 0)."""
    n = np.asarray(grid, np.float64)
    with np.errstate(invalid="ignore"):
        c = (points @ rot.T + trans + 1.0) * (n / 2) - 0.5
        ok = np.all((c > -1) & (c <= n), axis=1)
    ref0 = np.ceil(c[ok]).astype(np.int64) - 1
    shape = TILE[len(grid)]
    counts = np.zeros(tuple(-(-g // s) for g, s in zip(grid, shape)), np.int64)
    np.add.at(counts, tuple((np.maximum(ref0, 0) // np.asarray(shape)).T), 1)
    return counts


def heavy_tiles(counts, threshold):
    """(tiles above the threshold, face-adjacent pairs of them)"""
    heavy = counts > threshold
    pairs = 0
    for ax in range(heavy.ndim):
        a = np.moveaxis(heavy, ax, 0)
        pairs += int((a[1:] & a[:-1]).sum())
    return int(heavy.sum()), pairs


def poses(single):
    return (0,) if single else (0, 1, 2)


def elementwise(got, ref64, family, name, what):
    """The fp32 element-wise bound of the module docstring on one image-shaped plane."""
    g = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert g.shape == ref64.shape, f"{what}: shape {g.shape} != {ref64.shape}"
    scale = np.abs(ref64).max()
    rho = RHO[(family, name)]
    m = M_FACTOR * rho if rho > 0 else 8 * float(np.finfo(np.float32).eps)
    d = np.abs(g - ref64).max()
    print(f"{family} {name} {what}: max|got - ref64| / max|ref64| = {d / scale:.3e} (m = {m:.3e})")
    assert d <= m * scale, f"{what}: max|got - ref64| = {d:.3e} > {m:.3e} * {scale:.3e}"


# ------------------------------------------------------------------ 0. the regime is what the table says
@pytest.mark.parametrize("name", ["H3", "H2_22", "H2_32"])
def test_clustered_inputs_split_adjacent_tiles(name):
    """Every pose puts more than SPLIT records into at least two face-adjacent tiles -- a change of the generator
    cannot silently drop the regime.  3-D: SPLIT is twice the 4096 records asked for.  2-D: the identity pose 0 (the
    single-pose runs) centres the cluster on voxel (50, 35), mid-tile along x and 1.8 standard deviations above the
    tile edge at y = 32, so its second tile holds ~2900 records -- above the 2048 at which the 2-D path splits, below
    4096; the generator's seed is chosen so that poses 1 and 2 shift the cluster across a tile edge and load two
    adjacent tiles with more than 4096 each.  (Counting needs no device.)"""
    h = hard(name)
    for b in range(3):
        counts = tile_counts(h.grid, h.points, h.rot[b], h.trans[b])
        n_split, pairs = heavy_tiles(counts, SPLIT[h.n_out])
        n_4096, pairs_4096 = heavy_tiles(counts, 4096)
        print(f"{name} pose {b}: {counts.size} tiles, above {SPLIT[h.n_out]}: {n_split} ({pairs} adjacent pairs), "
              f"above 4096: {n_4096} ({pairs_4096} adjacent pairs), max {counts.max()}")
        assert n_split >= 2 and pairs >= 1, (name, b, n_split, pairs)
        if h.n_out == 3 or b > 0:
            assert n_4096 >= 2 and pairs_4096 >= 1, (name, b, n_4096, pairs_4096)


# ------------------------------------------------------------------ 1. JVP, TILED
@functools.lru_cache(maxsize=None)
def jvp_data(name, case):
    h = hard(name)
    rng = np.random.default_rng(SPEC[name][5] + 17)
    ow, pw, bg = r32(rng.uniform(0.5, 2.0, size=3)), r32(rng.uniform(0.5, 2.0, size=h.P)), r32(rng.normal(size=3))
    if case == "all":  # K = 3 tangents of all six kinds
        K, kinds = 3, KINDS
    else:  # K = 1 of point_weight only; the deposit ow * point_weight_dot of a point of weight 0 must not be lost
        K, kinds = 1, ("point_weight",)
        pw[::10] = 0.0
    tan = {k: r32(v) for k, v in random_tangents(rng, K, h.P, 3, h.n_in, h.n_out, kinds).items()}
    return SimpleNamespace(K=K, ow=ow, pw=pw, bg=bg, tan=tan)


@functools.lru_cache(maxsize=None)
def jvp_expected(name, case, cell_dtype, value_dtype=np.float64):
    h, j = hard(name), jvp_data(name, case)
    with np.errstate(invalid="ignore"):
        return jvp_reference(h.grid, h.points, h.rot, h.trans, j.ow, j.pw, j.tan, j.K, cell_dtype=cell_dtype,
                             value_dtype=value_dtype)


def run_jvp(h, j, tdt, dev, algo, single):
    t = lambda a: to(a, tdt, dev)
    kw = {}
    for kind, v in j.tan.items():
        if single and kind in ("rotation", "translation", "background", "out_weight"):
            v = v[:, 0]
        kw[kind + "_dot"] = t(v)
    s = (lambda a: a[0]) if single else (lambda a: a)
    s1 = (lambda a: a[:1]) if single else (lambda a: a)
    out = dpr_amd.raster_jvp(h.grid, t(h.points), t(s(h.rot)), t(s(h.trans)), t(s1(j.bg)), t(s1(j.ow)), t(j.pw),
                             **kw, tangents=j.K, algo=algo)
    assert tuple(out.shape) == tuple(h.grid) + (j.K,) + (() if single else (3,))
    return out.unsqueeze(-1) if single else out


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("case", ["all", "point_weight"])
@pytest.mark.parametrize("name", INPUTS)
def test_jvp_tiled(dev, name, case, npdt, tdt):
    h, j = hard(name), jvp_data(name, case)
    ref = jvp_expected(name, case, npdt)  # (the cells of the test's dtype, everything after them fp64)
    for single in (True, False):
        sel = list(poses(single))
        tiled = run_jvp(h, j, tdt, dev, "tiled", single)
        atomic = run_jvp(h, j, tdt, dev, "atomic", single)
        assert bool(torch.isfinite(tiled).all()), "non-finite out_dot"
        assert_close(tiled.double(), ref[..., sel], jvp_tol(npdt), f"{name} {case} single={single} vs restatement")
        assert_close(tiled.double(), atomic.double(), jvp_tol(npdt), f"{name} {case} single={single} vs atomic")
        if npdt == np.float32:
            for k in range(j.K):
                for i, b in enumerate(sel):
                    elementwise(tiled[..., k, i], ref[..., k, b], "jvp_" + case, name, f"out_dot[.., {k}, {b}]")


def test_jvp_tiled_adjoint_identity_h3_fp64(dev):
    """<J v, u> = <v, J^T u> with the ATOMIC pullback, as test_adjoint_identity_with_the_pullback."""
    h, j = hard("H3"), jvp_data("H3", "all")
    t = lambda a: to(a, torch.float64, dev)
    out = run_jvp(h, j, torch.float64, dev, "tiled", False)
    u = dpr_amd.to_grid_layout(torch.randn(tuple(h.grid) + (3,), dtype=torch.float64, device=dev,
                                           generator=torch.Generator(device=dev).manual_seed(3)))
    g = dpr_amd.raster_pullback_(u, t(h.points), t(h.rot), t(h.trans), t(j.bg), t(j.ow), t(j.pw), algo="atomic")
    grads = dict(points=g.points, rotation=g.rotation, translation=g.translation, background=g.background,
                 out_weight=g.out_weight, point_weight=g.point_weight)
    for k in range(j.K):
        lhs = float((out[..., k, :] * u).sum())
        rhs = sum(float((t(j.tan[kind][k]) * grads[kind]).sum()) for kind in KINDS)
        scale = float(out[..., k, :].norm() * u.norm())
        assert abs(lhs - rhs) <= 1e-11 * scale, (k, lhs, rhs)


# ------------------------------------------------------------------ 2. channels, TILED (and the ATOMIC pullback)
@functools.lru_cache(maxsize=None)
def channel_data(name):
    """16 channels (a test of C channels takes the first C); channel 1 is zero on half of the points."""
    h = hard(name)
    rng = np.random.default_rng(SPEC[name][5] + 100)
    pw = rng.uniform(0.2, 1.0, size=(h.P, 16)) * (1.0 + np.arange(16))
    pw[rng.permutation(h.P)[: h.P // 2], 1] = 0.0
    return SimpleNamespace(pw=r32(pw), bg=r32(rng.uniform(-1, 1, size=(3, 16))), ow=r32(rng.uniform(0.5, 2.0, size=3)),
                           ds=r32(rng.normal(size=h.grid + (16, 3))))


def channel_problem(h, ch, C, tdt, dev, single):
    """The dict of tests/test_channels_gpu.py's `problem`."""
    t = lambda a: to(a, tdt, dev)
    p = dict(points=t(h.points), pw=t(ch.pw[:, :C]), grid=h.grid)
    if single:
        p.update(rot=t(h.rot[0]), trans=t(h.trans[0]), bg=t(ch.bg[0, :C]), ow=float(ch.ow[0]))
    else:
        p.update(rot=t(h.rot), trans=t(h.trans), bg=t(ch.bg[:, :C]), ow=t(ch.ow))
    return p


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("name", INPUTS)
def test_channels_tiled(dev, name, C, npdt, tdt):
    h, ch = hard(name), channel_data(name)
    for single in (True, False):
        p = channel_problem(h, ch, C, tdt, dev, single)
        out = dpr_amd.raster_channels(h.grid, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                      algo="tiled")
        assert tuple(out.shape) == tuple(h.grid) + (C,) + (() if single else (3,))
        assert bool(torch.isfinite(out).all()), "non-finite out"
        for c in range(C):
            got = plane(out, c, h.n_out)
            assert_close(got, oracle_plane(p, c, npdt), tol(npdt, "out"), f"{name} single={single} plane {c}")
            if npdt == np.float32:
                ref64 = oracle_plane(p, c, np.float64)
                for i, b in enumerate(poses(single)):
                    elementwise(got if single else got[..., i], ref64 if single else ref64[..., i], "channels",
                                name, f"out[.., {c}, {b}]")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("name", INPUTS)
def test_channels_atomic_pullback(dev, name, C, npdt, tdt):
    """The channel pullback has no tiled form; out-of-grid, face and NaN / Inf points with C > 1 are new to it."""
    h, ch = hard(name), channel_data(name)
    for single in (True, False):
        sel = list(poses(single))
        p = channel_problem(h, ch, C, tdt, dev, single)
        g = dpr_amd.empty_channel_grid(h.grid, C, None if single else 3, tdt, dev)
        ds = ch.ds[..., :C, :]
        g.copy_(to(ds[..., 0] if single else ds, tdt, dev))
        pb = dpr_amd.raster_pullback_channels_(g, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"],
                                               algo="atomic")
        torch.cuda.synchronize()
        sums = None
        for c in range(C):
            r = oracle.raster_pullback(ds[..., c, sel], h.points, h.rot[sel], h.trans[sel], ch.ow[sel], ch.pw[:, c],
                                       dtype=npdt)
            assert_close(pb.point_weight[:, c], r.point_weight, tol(npdt, "points"), f"ds_dpoint_weight[:, {c}]")
            assert_close(pb.background[..., c].reshape(-1), r.background, tol(npdt, "pose"),
                         f"ds_dbackground[.., {c}]")
            parts = [np.asarray(x, np.float64) for x in (r.points, r.rotation, r.translation, r.out_weight)]
            sums = parts if sums is None else [s + x for s, x in zip(sums, parts)]
        first = (lambda a: a[0]) if single else (lambda a: a)
        assert_close(pb.points, sums[0], tol(npdt, "points"), "ds_dpoints")
        assert_close(pb.rotation, first(sums[1]), tol(npdt, "pose"), "ds_drotation")
        assert_close(pb.translation, first(sums[2]), tol(npdt, "pose"), "ds_dtranslation")
        assert_close(pb.out_weight.reshape(-1), sums[3], tol(npdt, "pose"), "ds_dout_weight")
        for x in pb:
            assert bool(torch.isfinite(x).all())


# ------------------------------------------------------------------ 3. sampling
@functools.lru_cache(maxsize=None)
def sample_data(name):
    h = hard(name)
    rng = np.random.default_rng(SPEC[name][5] + 200)
    return SimpleNamespace(image=r32(rng.normal(size=h.grid + (3,))), dv=r32(rng.normal(size=(h.P, 3))))


def check_sample_pullback(pb, grid, points, rot, trans, image, dv, npdt, single, ew=None):
    """The per-pose oracle composition of test_pullback_matches_per_pose_oracle_calls: ds_dimage[.., b] is the
    raster of weights ds_dvalues[:, b], the geometric gradients are raster_pullback's with those weights."""
    B = rot.shape[0]
    sum_pts = np.zeros_like(points)
    for b in range(B):
        R, t = rot[b:b + 1], trans[b:b + 1]
        if pb.image is not None:
            got_img = pb.image if single else pb.image[..., b]
            ref_img = oracle.raster(grid, points, R, t, None, None, dv[:, b], dtype=npdt)[..., 0]
            assert_close(got_img, ref_img, tol(npdt, "out"), f"ds_dimage[.., {b}]")
            if ew is not None:
                ref64 = oracle.raster(grid, points, R, t, None, None, dv[:, b], dtype=np.float64)[..., 0]
                elementwise(got_img, ref64, "sample", ew, f"ds_dimage[.., {b}]")
        r = oracle.raster_pullback(image[..., b:b + 1], points, R, t, np.ones(1), dv[:, b], dtype=npdt)
        assert_close(pb.rotation if single else pb.rotation[b], r.rotation[0], tol(npdt, "pose"), f"ds_drotation[{b}]")
        assert_close(pb.translation if single else pb.translation[b], r.translation[0], tol(npdt, "pose"),
                     f"ds_dtranslation[{b}]")
        sum_pts += r.points
    assert_close(pb.points, sum_pts, tol(npdt, "points"), "ds_dpoints")
    for x in pb:
        assert x is None or bool(torch.isfinite(x).all())


@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name", ["H3", "H2_22", "H2_32"])
def test_sample_pullback(dev, name, algo, npdt, tdt):
    h, s = hard(name), sample_data(name)
    t = lambda a: to(a, tdt, dev)
    img = dpr_amd.to_grid_layout(t(s.image))
    for single in (True, False):
        sel = list(poses(single))
        if single:
            pb = dpr_amd.sample_pullback_(t(s.dv[:, 0]), img[..., 0], t(h.points), t(h.rot[0]), t(h.trans[0]),
                                          algo=algo)
        else:
            pb = dpr_amd.sample_pullback_(t(s.dv), img, t(h.points), t(h.rot), t(h.trans), algo=algo)
        torch.cuda.synchronize()
        check_sample_pullback(pb, h.grid, h.points, h.rot[sel], h.trans[sel], s.image[..., sel], s.dv[:, sel], npdt,
                              single, ew=name if npdt == np.float32 else None)


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_pose_slices_of_the_direct_kernels(dev, npdt, tdt):
    """k_sample_fwd, k_sample_bwd and k_jvp_atomic walk the poses in slices (pose_slices of csrc/dpr_host.h):
    P = 40 000 is pblocks = ceil(40000 / 256) = 157 blocks of points, under 2048, so the poses are sliced:
    slices = ceil(2048 / 157) = 14 (not above B = 37), poses per slice = ceil(37 / 14) = 3, slices =
    ceil(37 / 3) = 13 -- twelve slices of three poses and a last slice of one."""
    P, B, K, grid = 40_000, 37, 2, (40, 40)
    pblocks = -(-P // 256)
    slices = min(-(-2048 // pblocks), B)
    per_slice = -(-B // slices)
    assert (pblocks, slices, per_slice, -(-B // per_slice), B - 12 * per_slice) == (157, 14, 3, 13, 1)
    d = D.make(n_points=P, n_in=3, n_out=2, batch=B, grid_n=grid, seed=31)
    rng = np.random.default_rng(32)
    pts, rot, trans = r32(d.points), r32(d.rotations), r32(d.translations)
    pts[::100] *= 4.0  # some outside the grid
    pts = r32(pts)
    image, dv = r32(rng.normal(size=grid + (B,))), r32(rng.normal(size=(P, B)))
    t = lambda a: to(a, tdt, dev)
    img = dpr_amd.to_grid_layout(t(image))
    v = dpr_amd.sample(img, t(pts), t(rot), t(trans))
    pb = dpr_amd.sample_pullback_(t(dv), img, t(pts), t(rot), t(trans), algo="atomic")
    torch.cuda.synchronize()
    assert v.shape == (P, B)
    for b in range(B):
        ref = oracle.raster_pullback(image[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1], np.ones(1),
                                     dtype=npdt).point_weight
        assert_close(v[:, b], ref, tol(npdt, "out"), f"values[:, {b}]")
    # no sum across poses in `sample`: the one pose of the partial last slice equals its own single-pose call
    last = dpr_amd.sample(img[..., B - 1], t(pts), t(rot[B - 1]), t(trans[B - 1]))
    assert torch.equal(v[:, B - 1], last)
    check_sample_pullback(pb, grid, pts, rot, trans, image, dv, npdt, False)
    ow, pw = r32(rng.uniform(0.5, 2.0, size=B)), r32(rng.uniform(0.5, 2.0, size=P))
    tan = {k: r32(x) for k, x in random_tangents(rng, K, P, B, 3, 2, KINDS).items()}
    out = dpr_amd.raster_jvp(grid, t(pts), t(rot), t(trans), t(np.zeros(B)), t(ow), t(pw), tangents=K, algo="atomic",
                             **{k + "_dot": t(x) for k, x in tan.items()})
    ref = jvp_reference(grid, pts, rot, trans, ow, pw, tan, K, cell_dtype=npdt)
    assert tuple(out.shape) == grid + (K, B)
    for b in range(B):
        assert_close(out[..., b].double(), ref[..., b], jvp_tol(npdt), f"out_dot[.., {b}]")


# ------------------------------------------------------------------ 4. per-pose clouds, TILED
@functools.lru_cache(maxsize=None)
def hard_clouds():
    """Three clouds of 40 000 points on the H3 grid: 0 and 2 clustered (split tiles), 1 diffuse (no tile above the
    4096 records at which the pullback would split it); F in cloud 0; uneven sizes padded with zero weights as in
    tests/test_clouds_gpu.py's `clouds`."""
    grid, B, P, seed = SPEC["H3"][2], 3, 40_000, 41
    rng = np.random.default_rng(seed)
    d = D.make(n_points=4, n_in=3, n_out=3, batch=B, grid_n=grid, seed=seed)
    rot, trans = d.rotations.copy(), d.translations.copy()
    rot[0] = np.eye(3)
    trans[0] = 0.0
    pts = 0.4 * rng.normal(size=(B, P, 3))
    for b in (0, 2):
        pts[b] *= 0.12
        pts[b, ::50] *= 8.0
    pts[1, ::50] *= 4.0
    f = face_and_bad_points(rng, 3, 3, grid)
    pts[0, :len(f)] = f
    pw = rng.uniform(0.5, 1.5, size=(B, P))
    for b in range(B):
        pw[b, P - (b * P) // (2 * B):] = 0.0
    return dict(grid=grid, points=r32(pts), rot=r32(rot), trans=r32(trans), pw=r32(pw),
                bg=np.arange(1, B + 1, dtype=np.float64), ow=r32(rng.uniform(1, 10, size=B)),
                ds=r32(rng.normal(size=grid + (B,))), B=B, P=P)


def test_hard_clouds_split_tiles_in_clouds_0_and_2_only():
    c = hard_clouds()
    for b in range(3):
        counts = tile_counts(c["grid"], c["points"][b][c["pw"][b] != 0], c["rot"][b], c["trans"][b])
        n_heavy, pairs = heavy_tiles(counts, SPLIT[3])
        print(f"cloud {b}: {counts.size} tiles, {n_heavy} heavy, {pairs} adjacent pairs, max {counts.max()}")
        if b == 1:
            full = tile_counts(c["grid"], c["points"][b], c["rot"][b], c["trans"][b])
            assert full.max() <= 4096, full.max()
        else:
            assert n_heavy >= 2 and pairs >= 1, (b, n_heavy, pairs)


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_clouds_tiled(dev, npdt, tdt):
    c = hard_clouds()
    t = clouds_on(dev, tdt, c)
    B, P, grid = c["B"], c["P"], c["grid"]
    ws = torch.empty(max(dpr_amd.workspace_bytes_clouds(op, grid, P, B, 3, tdt, "tiled") for op in
                         ("raster", "pullback")), dtype=torch.uint8, device=dev)
    args = (t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"])
    first = None
    for run in range(2):  # the second call finds what pose 2's split tiles left in the workspace
        out = dpr_amd.empty_grid(grid, B, tdt, dev).fill_(float("nan"))
        nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=dev)
        bufs = dict(ds_dpoints=nan(B, P, 3), ds_drotation=nan(B, 3, 3).transpose(1, 2), ds_dtranslation=nan(B, 3),
                    ds_dbackground=nan(B), ds_dout_weight=nan(B), ds_dpoint_weight=nan(B, P))
        dpr_amd.raster_clouds_(out, *args, algo="tiled", workspace=ws)
        pb = dpr_amd.raster_pullback_clouds_(t["ds"], *args, algo="tiled", workspace=ws, **bufs)
        torch.cuda.synchronize()
        for x in (out, *pb):
            assert bool(torch.isfinite(x).all()), f"run {run}: an output keeps NaN"
        check_against_oracle(c, out, pb, npdt)
        if npdt == np.float32:
            for b in range(B):
                ref64 = oracle.raster(grid, c["points"][b], c["rot"][b:b + 1], c["trans"][b:b + 1], c["bg"][b:b + 1],
                                      c["ow"][b:b + 1], c["pw"][b], dtype=np.float64)[..., 0]
                elementwise(out[..., b], ref64, "clouds", "H3", f"run {run} out[.., {b}]")
        if first is None:
            first = (out, pb)
    if npdt == np.float32:
        out, pb = first
        for b in range(B):
            one = (grid, t["points"][b], t["rot"][b], t["trans"][b], t["bg"][b], t["ow"][b], t["pw"][b])
            ref = dpr_amd.raster(*one, algo="tiled")
            rerun = dpr_amd.raster(*one, algo="tiled")
            _bit_equal_or_rounding(out[..., b], ref, rerun, f"plane {b}")
            p1 = dpr_amd.raster_pullback_(t["ds"][..., b], *one[1:], algo="tiled")
            torch.cuda.synchronize()
            assert torch.equal(pb.points[b], p1.points), b
            assert torch.equal(pb.point_weight[b], p1.point_weight), b
