"""GPU tests of the BASELINE.json configurations at their stated one-GPU sizes, of the plain
(non-`_ex`) C entry points exactly as INTEGRATION.md binds them, of AUTO at a size where it
picks the tiled pipeline against the oracle (with the SURVEY.md 8(c) flip report), and of the
sharded drivers with the real HIP local compute under an RCCL ("nccl") process group."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests.conftest import ROOT
from tests.test_parity_gpu import T, _ball_points, _compare, assert_close, grid_to_dev, tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()  # fail loudly if the extension is missing: there is no fallback
    return torch.device("cuda:0")


# ------------------------------------------------------------------ C1, literally
@pytest.mark.parametrize("algo", ["auto", "atomic", "tiled", "chunked"])
def test_c1_1k_points_5x5_identity(oracle, dev, algo):
    """BASELINE.json configs[0]: 1 000 random 2-D points -> 5x5 grid, identity pose, fp64,
    raster + raster_pullback! against the oracle (src/raster.jl:5-34, raster_pullback.jl:2-82)."""
    rng = np.random.default_rng(0)
    pts = 0.4 * rng.standard_normal(size=(1000, 2))
    R, t = np.eye(2)[None], np.zeros((1, 2))
    g = np.asfortranarray(rng.normal(size=(5, 5, 1)))
    ref = oracle.raster((5, 5), pts, R, t)
    rpb = oracle.raster_pullback(g, pts, R, t)
    out = dpr_amd.raster((5, 5), T(pts, dev), T(R[0], dev), T(t[0], dev), algo=algo)
    pb = dpr_amd.raster_pullback_(grid_to_dev(g[..., 0], dev), T(pts, dev), T(R[0], dev),
                                  T(t[0], dev), algo=algo)
    assert_close(out, ref[..., 0], 1e-10, "out")
    assert_close(pb.points, rpb.points, 1e-10, "ds_dpoints")
    assert_close(pb.rotation, rpb.rotation[0], 1e-10, "ds_drotation")
    assert_close(pb.translation, rpb.translation[0], 1e-10, "ds_dtranslation")
    assert_close(pb.point_weight, rpb.point_weight, 1e-10, "ds_dpoint_weight")
    assert abs(float(pb.background) - rpb.background[0]) <= 1e-10 * abs(rpb.background[0])
    assert abs(float(pb.out_weight) - rpb.out_weight[0]) <= 1e-10 * abs(rpb.out_weight[0])


# ------------------------------------------------------------------ C4 at its one-GPU share
def test_c4_share_64_poses(dev):
    """BASELINE.json configs[3] at the share one of 8 GPUs owns: 10 M points -> 512^2
    orthographic projections, 64 poses, fp32, AUTO.  Size-independent properties: mass per
    pose, a pose of the batch == the single-pose call, adjoint identity
    <g, out - bg> = ow * d/d(ow) per pose, ds_dbackground = sum(ds_dout)."""
    P, n, B = 10_000_000, 512, 64
    # the path this test is meant to cover: AUTO must resolve to the chunk-owner algorithm here
    # (a cost-model edit that moved C4 back to the tiled path would otherwise pass unnoticed)
    assert dpr_amd.resolve_algo("raster", (n, n), P, B, 3) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (n, n), P, B, 3) == "chunked"
    f32 = dict(device=dev, dtype=torch.float32)
    pts = _ball_points(P, dev, torch.float32)
    rng = np.random.default_rng(5)
    R = T(D.random_rotations(rng, B)[:, :2, :].astype(np.float32), dev)
    t = T((0.05 * rng.normal(size=(B, 2))).clip(-0.1, 0.1).astype(np.float32), dev)
    ow = torch.linspace(0.5, 2.0, B, **f32)
    bg = torch.linspace(-1.0, 1.0, B, **f32)
    out = dpr_amd.raster((n, n), pts, R, t, bg, ow)
    sums = out.double().sum(dim=(0, 1)).cpu().numpy()
    expect = ow.double().cpu().numpy() * P + bg.double().cpu().numpy() * n * n
    np.testing.assert_allclose(sums, expect, rtol=2e-4)
    for b in (0, 37, 63):
        single = dpr_amd.raster((n, n), pts, R[b], t[b], float(bg[b]), float(ow[b]))
        assert_close(out[..., b], single.cpu().numpy(), 2e-5, f"pose {b} of the batch vs single call")
    g = torch.randn(B, n, n, **f32).permute(2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, bg, ow)
    lhs = (g.double() * (out.double() - bg.double())).sum(dim=(0, 1)).cpu().numpy()
    rhs = (ow.double() * pb.out_weight.double()).cpu().numpy()
    np.testing.assert_allclose(lhs, rhs, rtol=2e-3, atol=2e-3 * np.sqrt(P))
    np.testing.assert_allclose(pb.background.double().cpu().numpy(),
                               g.double().sum(dim=(0, 1)).cpu().numpy(), rtol=0, atol=1e-3 * n)
    # batch == sum over a loop of single-pose pullbacks (test/util.jl:26-34), on 3 poses
    sub = [5, 21, 50]
    pb_sub = dpr_amd.raster_pullback_(dpr_amd.to_grid_layout(g[..., sub]), pts, R[sub], t[sub],
                                      bg[sub], ow[sub])
    acc = torch.zeros_like(pb_sub.points)
    for k, b in enumerate(sub):
        one = dpr_amd.raster_pullback_(dpr_amd.to_grid_layout(g[..., b]), pts, R[b], t[b],
                                       float(bg[b]), float(ow[b]))
        acc += one.points
        assert_close(pb_sub.rotation[k], one.rotation.cpu().numpy(), 1e-3, "ds_drotation")
    assert_close(pb_sub.points, acc.cpu().numpy(), 1e-4, "batched ds_dpoints == sum of singles")


# ------------------------------------------------------------------ C5 at its one-GPU share
def test_c5_share_8_poses(dev):
    """BASELINE.json configs[4] at the share one of 8 GPUs owns: 50 M points -> 512^3 fp64,
    8 poses (out and ds_dout: 8.6 GB each).  Mass per pose, constant-sensitivity pullback,
    adjoint identity per pose."""
    P, n, B = 50_000_000, 512, 8
    f64 = dict(device=dev, dtype=torch.float64)
    pts = _ball_points(P, dev, torch.float64, seed=3)
    rng = np.random.default_rng(2)
    R = T(D.random_rotations(rng, B), dev)
    t = T((0.05 * rng.normal(size=(B, 3))).clip(-0.1, 0.1), dev)
    ow = torch.linspace(0.5, 1.5, B, **f64)
    out = dpr_amd.raster((n, n, n), pts, R, t, None, ow)
    for b in range(B):
        assert abs(float(out[..., b].sum()) - float(ow[b]) * P) <= 1e-9 * P
    g = torch.randn(B, n, n, n, **f64).permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, None, ow)
    for b in range(B):
        gb = g[..., b]
        assert abs(float(pb.background[b]) - float(gb.sum())) <= 1e-8 * float(gb.abs().sum())
        lhs = float((gb * out[..., b]).sum())
        rhs = float(ow[b]) * float(pb.out_weight[b])
        assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), 1.0)
    del out
    g.fill_(0.5)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, None, ow)
    assert float(pb.points.abs().max()) <= 1e-9 * n * B
    assert_close(pb.point_weight, np.full(P, 0.5 * float(ow.sum())), 1e-12)


def test_c5_full_job_64_poses_of_50m_points_on_one_gpu(dev):
    """BASELINE.json configs[4] as ONE job on one GPU -- the N = 1 anchor of its scaling curve: 50 M points ->
    512^3 fp64, all 64 poses in one call each way (`out` and `ds_dout`: 68.7 GB each; with the workspace
    ~165 GB of the 288).  Too large for the oracle: size-independent properties per pose -- mass (every
    point of the ball lands inside the grid under every pose: sum(out[b]) = out_weight[b] * P), the
    background sensitivity (= sum of ds_dout[b]), the adjoint identity <ds_dout[b], out[b]> = out_weight[b]
    * ds_dout_weight[b] (the forward is linear in out_weight) -- and a constant sensitivity, whose point
    gradients vanish while ds_dpoint_weight = 0.5 * sum(out_weight)."""
    P, n, B = 50_000_000, 512, 64
    free, _total = torch.cuda.mem_get_info(dev)
    if free < 200e9:
        pytest.skip(f"needs ~170 GB of device memory, {free / 1e9:.0f} GB free")
    f64 = dict(device=dev, dtype=torch.float64)
    pts = _ball_points(P, dev, torch.float64, seed=5)
    rng = np.random.default_rng(6)
    R = T(D.random_rotations(rng, B), dev)
    t = T((0.05 * rng.normal(size=(B, 3))).clip(-0.1, 0.1), dev)
    ow = torch.linspace(0.5, 1.5, B, **f64)
    out = dpr_amd.raster((n, n, n), pts, R, t, None, ow)
    mass = out.sum(dim=(0, 1, 2))
    assert float((mass - ow * P).abs().max()) <= 1e-9 * P
    g = torch.empty(B, n, n, n, **f64)
    gen = torch.Generator(device=dev).manual_seed(7)
    for b in range(B):
        g[b].normal_(generator=gen)
    g = g.permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, None, ow)
    for b in range(0, B, 7):  # (every seventh pose: each check reads 2 x 1 GB)
        gb = g[..., b]
        assert abs(float(pb.background[b]) - float(gb.sum())) <= 1e-8 * float(gb.abs().sum())
        lhs = float((gb * out[..., b]).sum())
        rhs = float(ow[b]) * float(pb.out_weight[b])
        assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), 1.0), b
    assert bool(torch.isfinite(pb.points).all()) and bool(torch.isfinite(pb.rotation).all())
    del out
    torch.cuda.empty_cache()
    g.fill_(0.5)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, None, ow)
    assert float(pb.points.abs().max()) <= 1e-9 * n * B
    assert float((pb.point_weight - 0.5 * float(ow.sum())).abs().max()) <= 1e-10 * B


@pytest.mark.parametrize("n_points,n_in,n_out,batch,grid_n", [
    (500, 3, 3, 1, 8),          # AUTO -> atomic: nothing to keep, the flags are ignored
    (300_000, 3, 3, 1, 64),     # AUTO -> tiled for both calls, shared binning
    (30_000, 3, 3, 3, 40),      # a batch on a 3-D grid: no sharing, each call on its own
    (150_000, 3, 2, 12, 96),    # AUTO -> chunk-owner pair (the sorted copy is shared)
    (400, 2, 2, 2, 16),
    (60_000, 3, 2, 40, 300),    # sparse cloud, many poses: wide footprints
])
def test_auto_accepts_keep_and_reuse_for_any_problem(oracle, dev, n_points, n_in, n_out, batch, grid_n):
    """include/dpr.h, dpr_resolve_algo_ex: a caller (the rrule) may always pass AUTO + KEEP_BINNING
    to raster and AUTO + REUSE_BINNING to the pullback of the same arguments; AUTO picks one
    algorithm for the pair or ignores the flags -- never an error, never stale lists."""
    d = D.make(n_points=n_points, n_in=n_in, n_out=n_out, batch=batch, grid_n=grid_n, seed=21,
               dtype=np.float32)
    args = (T(d.points, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev),
            T(d.weights, dev), T(d.point_weights, dev))
    need = max(dpr_amd.workspace_bytes(op, d.grid, n_points, batch, n_in, torch.float32, "auto", sharing=True)
               for op in ("raster", "pullback"))
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)
    pair = {dpr_amd.resolve_algo(op, d.grid, n_points, batch, n_in, sharing=True) for op in ("raster", "pullback")}
    assert len(pair) == 1 or "chunked" not in pair
    out = dpr_amd.empty_grid(d.grid, batch, torch.float32, dev)
    g = grid_to_dev(d.ds_dout, dev)
    dpr_amd.raster_(out, *args, algo="auto", workspace=ws, keep_binning=True)
    pb = dpr_amd.raster_pullback_(g, *args, algo="auto", workspace=ws, reuse_binning=True)
    ref_out = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                            d.point_weights, dtype=np.float32)
    ref_pb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights,
                                    d.point_weights, dtype=np.float32)
    _compare(ref_out, ref_pb, out, pb, np.float32)


def chunk_owner_fuzz_case(oracle, dev, seed):
    """One seeded case of DPR_ALGO_CHUNKED on a 2-D grid against the oracle: cloud sizes around the
    chunk / slice boundaries, anisotropic images from tiny to sparse (wide footprints: the
    work-list kernel), 1 ... 70 poses (pose slices), both point dimensions and element types,
    optional arguments, NaN points, scaled "rotations" (the footprint bound must hold for any
    matrix), pre-sorted input with the coherence flag, keep / reuse.  tools/fuzz_chunkown.py runs
    hundreds of seeds."""
    from tests.test_parity_gpu import DTYPES
    rng = np.random.default_rng(9000 + seed)
    n_in = int(rng.choice([2, 3]))
    npdt, tdt = DTYPES[rng.integers(2)]
    P = int(rng.choice([1, 700, 4095, 4096, 4097, 8193, 30_000, 120_001, 300_000]))
    B = int(rng.choice([1, 2, 5, 16, 33, 64, 70]))
    if P * B > 6_000_000:
        B = max(1, 6_000_000 // P)
    grid = (int(rng.choice([3, 17, 64, 150, 512, 900])), int(rng.choice([4, 31, 128, 333, 700])))
    spread = float(rng.choice([0.02, 0.4, 1.5]))
    pts = (spread * rng.normal(size=(P, n_in))).astype(npdt)
    if seed % 5 == 0 and P > 10:
        pts[:: max(1, P // 7)] = np.nan
    R = D.random_rotations(rng, B, n_in)[:, :2, :].astype(npdt)
    if seed % 4 == 0:
        R *= float(rng.choice([0.3, 2.5]))
    t = (float(rng.choice([0.0, 0.2, 1.1])) * rng.normal(size=(B, 2))).astype(npdt)
    use = rng.integers(0, 2, size=3).astype(bool)
    bg = rng.normal(size=B).astype(npdt) if use[0] else None
    ow = rng.uniform(0.5, 3, size=B).astype(npdt) if use[1] else None
    pw = rng.uniform(0.1, 2, size=P).astype(npdt) if use[2] else None
    g = np.asfortranarray(rng.normal(size=grid + (B,)).astype(npdt))
    mode = ["plain", "coherent", "keep_reuse"][seed % 3]
    ref_out = oracle.raster(grid, pts, R, t, bg, ow, pw, dtype=npdt)
    ref_pb = oracle.raster_pullback(g, pts, R, t, ow, pw, dtype=npdt)
    dp, dR, dt_, dbg, dow, dpw = (T(x, dev) for x in (pts, R, t, bg, ow, pw))
    perm, kw = None, {}
    if mode == "coherent":
        if pw is not None:
            dp, perm, dpw = dpr_amd.sort_points(dp, dpw)
        else:
            dp, perm = dpr_amd.sort_points(dp)
        kw = dict(coherent_points=True)
    need = max(16, *(dpr_amd.workspace_bytes(op, grid, P, B, n_in, tdt, "chunked", **kw)
                     for op in ("raster", "pullback")))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(grid, B, tdt, dev)
    dpr_amd.raster_(out, dp, dR, dt_, dbg, dow, dpw, algo="chunked", workspace=ws,
                    keep_binning=(mode == "keep_reuse"), **kw)
    pb = dpr_amd.raster_pullback_(grid_to_dev(g, dev), dp, dR, dt_, dbg, dow, dpw, algo="chunked",
                                  workspace=ws, reuse_binning=(mode == "keep_reuse"), **kw)
    if perm is not None:
        bp = torch.empty_like(pb.points)
        bp.index_copy_(0, perm.long(), pb.points)
        bw = torch.empty_like(pb.point_weight)
        bw.index_copy_(0, perm.long(), pb.point_weight)
        pb = pb._replace(points=bp, point_weight=bw)
    try:
        _compare(ref_out, ref_pb, out, pb, npdt)
    except AssertionError as e:
        raise AssertionError(f"{dict(seed=seed, P=P, B=B, grid=grid, n_in=n_in, dt=str(tdt), mode=mode)}: {e}")


@pytest.mark.parametrize("seed", range(16))
def test_chunk_owner_fuzz(oracle, dev, seed):
    chunk_owner_fuzz_case(oracle, dev, seed)


@pytest.mark.parametrize("residual", [False, True])
def test_chunk_owner_pullback_pipeline_over_mixed_poses(oracle, dev, residual):
    """The fp32 chunk-owner pullback prefetches the next pose's footprint into a second LDS tile
    while it gathers the current one.  One pose slice that alternates the three kinds of footprint
    the loop tells apart -- fits the tile (prefetched), empty (the chunk projects outside the
    image: nothing staged, sums stay 0) and too large for the tile (gathered from global memory) --
    in every order of succession, with and without the fused residual."""
    rng = np.random.default_rng(77)
    P, grid = 3 * 4096 + 100, (200, 160)
    pts = (0.05 * rng.normal(size=(P, 3)) + np.array([0.2, -0.1, 0.3])).astype(np.float32)
    kinds = [0, 1, 2, 0, 2, 1, 1, 0, 0, 2, 2, 1, 0]  # 0 fits, 1 outside, 2 blown up
    B = len(kinds)
    R = D.random_rotations(rng, B, 3)[:, :2, :].astype(np.float32)
    t = (0.05 * rng.normal(size=(B, 2))).astype(np.float32)
    for b, k in enumerate(kinds):
        if k == 1:
            t[b] += 3.0           # everything beyond the image
        if k == 2:
            R[b] *= 14.0          # a 4096-point chunk spreads over more than 8192 pixels
            t[b] -= (R[b] @ np.array([0.2, -0.1, 0.3], np.float32))  # ... centred on the image
    ow = rng.uniform(0.5, 2, size=B).astype(np.float32)
    pw = rng.uniform(0.2, 2, size=P).astype(np.float32)
    g = np.asfortranarray(rng.normal(size=grid + (B,)).astype(np.float32))
    dp, dR, dt_, dow, dpw = (T(x, dev) for x in (pts, R, t, ow, pw))
    if not residual:
        ref = oracle.raster_pullback(g, pts, R, t, ow, pw, dtype=np.float32)
        pb = dpr_amd.raster_pullback_(grid_to_dev(g, dev), dp, dR, dt_, None, dow, dpw, algo="chunked")
    else:
        out = oracle.raster(grid, pts, R, t, None, ow, pw, dtype=np.float32)
        ref = oracle.raster_pullback(np.asfortranarray(2.0 * (out - g)), pts, R, t, ow, pw, dtype=np.float32)
        pb, loss = dpr_amd.raster_residual_pullback_(grid_to_dev(np.asfortranarray(out), dev),
                                                     grid_to_dev(g, dev), dp, dR, dt_, None, dow, dpw,
                                                     scale=2.0, algo="chunked")
        assert_close(loss, ((out.astype(np.float64) - g) ** 2).sum(axis=(0, 1)), 1e-5, "loss")
    assert float(np.abs(ref.rotation[[b for b, k in enumerate(kinds) if k == 1]]).max()) == 0.0
    assert float(np.abs(ref.rotation[[b for b, k in enumerate(kinds) if k == 2]]).max()) > 0.0
    for name, kind in (("points", "points"), ("point_weight", "points"), ("rotation", "pose"),
                       ("translation", "pose"), ("out_weight", "pose")):
        assert_close(getattr(pb, name), getattr(ref, name), tol(np.float32, kind), name)


@pytest.mark.parametrize("npdt,tdt", [(np.float32, torch.float32), (np.float64, torch.float64)])
@pytest.mark.parametrize("with_pw", [False, True])
def test_chunk_owner_keeps_the_sorted_cloud_for_the_pullback(oracle, dev, npdt, tdt, with_pw):
    """DPR_ALGO_CHUNKED on a 2-D grid, batch of poses: the forward (KEEP_BINNING) leaves the
    Hilbert-sorted copy of the cloud in the workspace, the pullback (REUSE_BINNING) skips its own
    sort; a pullback that finds no matching copy returns NaN; pre-sorted input with
    coherent_points=True gives the same results."""
    d = D.make(n_points=120_000, n_in=3, n_out=2, batch=9, grid_n=96, seed=4, dtype=npdt)
    d.points[::11] *= 3.5  # some far outside
    pw = d.point_weights if with_pw else None
    args = (T(d.points, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev),
            T(d.weights, dev), T(pw, dev))
    ws = torch.zeros(dpr_amd.workspace_bytes("raster", d.grid, d.n_points, d.batch, 3, tdt, "chunked"),
                     dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, d.batch, tdt, dev)
    g = grid_to_dev(d.ds_dout, dev)
    ref_out = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                            pw, dtype=npdt)
    ref_pb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, pw,
                                    dtype=npdt)
    stale = dpr_amd.raster_pullback_(g, *args, algo="chunked", workspace=ws, reuse_binning=True)
    assert bool(torch.isnan(stale.points).all()) and bool(torch.isnan(stale.rotation).all())
    dpr_amd.raster_(out, *args, algo="chunked", workspace=ws, keep_binning=True)
    for _ in range(2):  # the sorted copy is not consumed
        pb = dpr_amd.raster_pullback_(g, *args, algo="chunked", workspace=ws, reuse_binning=True)
        _compare(ref_out, ref_pb, out, pb, npdt)
    other = T(d.points, dev).clone()
    wrong = dpr_amd.raster_pullback_(g, other, *args[1:], algo="chunked", workspace=ws, reuse_binning=True)
    assert bool(torch.isnan(wrong.points).all())
    # pre-sorted cloud + the coherence hint: no sort inside, same numbers
    if with_pw:
        sp, perm, spw = dpr_amd.sort_points(args[0], args[5])
    else:
        (sp, perm), spw = dpr_amd.sort_points(args[0]), None
    out2 = dpr_amd.raster(d.grid, sp, *args[1:5], spw, algo="chunked", coherent_points=True)
    assert_close(out2, ref_out, tol(npdt, "out"), "coherent forward")
    pb2 = dpr_amd.raster_pullback_(g, sp, *args[1:5], spw, algo="chunked", coherent_points=True)
    back = torch.empty_like(pb2.points)
    back.index_copy_(0, perm.long(), pb2.points)
    assert_close(back, ref_pb.points, tol(npdt, "points"), "coherent pullback through perm")
    assert_close(pb2.rotation, ref_pb.rotation, tol(npdt, "pose"), "coherent ds_drotation")


@pytest.mark.parametrize("npdt,tdt", [(np.float32, torch.float32), (np.float64, torch.float64)])
@pytest.mark.parametrize("n_in,n_out,grid_n", [(3, 3, 70), (3, 2, 150), (2, 2, 100)])
@pytest.mark.parametrize("order", ["sorted", "as generated"])
@pytest.mark.parametrize("with_pw", [False, True])
def test_local_binning_of_coherent_points(oracle, dev, npdt, tdt, n_in, n_out, grid_n, order, with_pw):
    """DPR_ALGO_TILED + DPR_FLAG_COHERENT_POINTS: sub-chunks are ordered by tile locally and the
    tile kernels walk run descriptors (no count pass, no global permutation).  Fast for sorted
    clouds, but the result must be right for ANY order (here also the generated, incoherent one),
    with points outside the grid, with the forward's binning kept for the pullback, and for a
    cluster dense enough to split tiles."""
    d = D.make(n_points=150_000, n_in=n_in, n_out=n_out, batch=2, grid_n=grid_n, seed=8, dtype=npdt)
    d.points[::13] *= 3.0          # some far outside
    d.points[1::5] *= 0.05         # a tight cluster: heavy tiles are split into parts
    pts, pw = T(d.points, dev), (T(d.point_weights, dev) if with_pw else None)
    perm = None
    if order == "sorted":
        if with_pw:
            pts, perm, pw = dpr_amd.sort_points(pts, pw)
        else:
            pts, perm = dpr_amd.sort_points(pts)
    pwn = d.point_weights if with_pw else None
    ref_out = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                            pwn, dtype=npdt)
    ref_pb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, pwn,
                                    dtype=npdt)
    pose = (T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev), T(d.weights, dev))
    # (a batch that can form pose groups stays on the grouped pipeline; one pose per group selects
    # the local bins for every pose of the batch)
    out = dpr_amd.raster(d.grid, pts, *pose, pw, algo="tiled", coherent_points=True, max_pose_group=1)
    assert_close(out, ref_out, tol(npdt, "out"), "out")
    out_g = dpr_amd.raster(d.grid, pts, *pose, pw, algo="tiled", coherent_points=True)
    assert_close(out_g, ref_out, tol(npdt, "out"), "out (grouped)")
    pb = dpr_amd.raster_pullback_(grid_to_dev(d.ds_dout, dev), pts, *pose, pw, algo="tiled",
                                  coherent_points=True, max_pose_group=1)
    def unsorted(x):
        if perm is None:
            return x
        back = torch.empty_like(x)
        back.index_copy_(0, perm.long(), x)
        return back
    assert_close(unsorted(pb.points), ref_pb.points, tol(npdt, "points"), "ds_dpoints")
    assert_close(unsorted(pb.point_weight), ref_pb.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
    assert_close(pb.rotation, ref_pb.rotation, tol(npdt, "pose"), "ds_drotation")
    assert_close(pb.translation, ref_pb.translation, tol(npdt, "pose"), "ds_dtranslation")
    assert_close(pb.out_weight, ref_pb.out_weight, tol(npdt, "pose"), "ds_dout_weight")
    # single pose: the pullback reuses what the forward kept
    ws = torch.empty(dpr_amd.workspace_bytes("raster", d.grid, d.n_points, 1, n_in, tdt, "tiled",
                                             coherent_points=True), dtype=torch.uint8, device=dev)
    o1 = dpr_amd.empty_grid(d.grid, None, tdt, dev)
    one = (pose[0][1], pose[1][1], float(d.backgrounds[1]), float(d.weights[1]))
    dpr_amd.raster_(o1, pts, *one, pw, algo="tiled", workspace=ws, keep_binning=True, coherent_points=True)
    assert_close(o1, ref_out[..., 1], tol(npdt, "out"), "kept forward")
    pb1 = dpr_amd.raster_pullback_(grid_to_dev(d.ds_dout[..., 1], dev), pts, *one, pw, algo="tiled",
                                   workspace=ws, reuse_binning=True, coherent_points=True)
    ref1 = oracle.raster_pullback(d.ds_dout[..., 1:2], d.points, d.rotations[1:2], d.translations[1:2],
                                  d.weights[1:2], pwn, dtype=npdt)
    assert_close(unsorted(pb1.points), ref1.points, tol(npdt, "points"), "reused ds_dpoints")
    assert_close(pb1.rotation, ref1.rotation[0], tol(npdt, "pose"), "reused ds_drotation")


def test_batched_large_grid_sorts_the_cloud_inside(oracle, dev, with_pw=True):
    """Batched poses on a grid with more than 4096 tiles: the tiled path cell-sorts the cloud
    into the workspace once per call (dpr_coarse.h), bins all poses locally, and brings the point
    gradients back through the inverse permutation.  250 k points -> 384 x 384 x 256 (4608 tiles), 4 poses, against the oracle."""
    npdt = np.float32
    d = D.make(n_points=250_000, n_in=3, n_out=3, batch=4, grid_n=384, seed=6, dtype=npdt)
    d.grid = (384, 384, 256)
    d.ds_dout = np.asfortranarray(d.ds_dout[:, :, :256, :])
    pw = d.point_weights if with_pw else None
    args = (T(d.points, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev),
            T(d.weights, dev), T(pw, dev))
    few = dpr_amd.workspace_bytes("raster", d.grid, d.n_points, 2, 3, torch.float32, "tiled")
    many = dpr_amd.workspace_bytes("raster", d.grid, d.n_points, 4, 3, torch.float32, "tiled")
    assert many > few + d.n_points * 12  # room for the sorted copy
    out = dpr_amd.raster(d.grid, *args, algo="tiled")
    ref_out = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                            pw, dtype=npdt)
    assert_close(out, ref_out, tol(npdt, "out"), "out")
    del out, ref_out
    pb = dpr_amd.raster_pullback_(grid_to_dev(d.ds_dout, dev), *args, algo="tiled")
    ref_pb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, pw,
                                    dtype=npdt)
    for name in ("points", "rotation", "translation", "background", "out_weight", "point_weight"):
        assert_close(getattr(pb, name), getattr(ref_pb, name),
                     tol(npdt, "points" if name.startswith("point") else "pose"), name)


@pytest.mark.parametrize("algo", ["auto", "tiled"])
def test_512_cube_fp64_vs_oracle(oracle, dev, algo):
    """HIP vs oracle on the C5 grid (512^3 fp64: 16384 tiles) with 1e5 points, all optional
    arguments given."""
    d = D.make(n_points=100_000, n_in=3, n_out=3, batch=1, grid_n=512, seed=21, dtype=np.float64)
    opt = (d.backgrounds, d.weights, d.point_weights)
    ref_out = oracle.raster(d.grid, d.points, d.rotations, d.translations, *opt)
    out = dpr_amd.raster(d.grid, T(d.points, dev), T(d.rotations, dev), T(d.translations, dev),
                         *[T(o, dev) for o in opt], algo=algo)
    assert_close(out, ref_out, 1e-10, "out")
    del ref_out, out
    ref_pb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, opt[1], opt[2])
    pb = dpr_amd.raster_pullback_(grid_to_dev(d.ds_dout, dev), T(d.points, dev), T(d.rotations, dev),
                                  T(d.translations, dev), *[T(o, dev) for o in opt], algo=algo)
    for name in ("points", "rotation", "translation", "background", "out_weight", "point_weight"):
        assert_close(getattr(pb, name), getattr(ref_pb, name), 1e-10, name)


# ------------------------------------------------------------------ AUTO -> tiled vs oracle, flip report
def _cell_flips(pts32, R, t, n):
    """Number of (point, axis) pairs whose cell choice ceil(coord - 1/2) differs between fp32
    and fp64 arithmetic on the same fp32 inputs (src/raster.jl:88-99 evaluated both ways)."""
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    proj = pts32[:, 0:1] * R32[:, 0][None]
    for j in range(1, pts32.shape[1]):
        proj = proj + pts32[:, j:j + 1] * R32[:, j][None]
    c32 = (proj - (np.float32(-1) - t32)) * np.float32(n / 2) - np.float32(0.5)
    c64 = ((pts32.astype(np.float64) @ R32.astype(np.float64).T) - (-1.0 - t32.astype(np.float64))) * (n / 2) - 0.5
    return int((np.ceil(c32) != np.ceil(c64)).sum())


def test_c2_full_size_auto_vs_oracle_with_flip_report(oracle, dev):
    """BASELINE.json configs[1] at full size (1 M points -> 128^3, fp32, one pose) with
    algo="auto" -- which resolves to the TILED pipeline here -- against the fp32 AND the fp64
    oracle; prints the SURVEY.md 8(c) report: max-abs errors and the number of fp32-vs-fp64
    cell-selection flips."""
    P, n = 1_000_000, 128
    assert dpr_amd.resolve_algo("raster", (n,) * 3, P, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (n,) * 3, P, 1, 3) == "tiled"
    rng = np.random.default_rng(0)
    pts = (0.4 * rng.standard_normal(size=(P, 3), dtype=np.float32))
    R = D.random_rotations(np.random.default_rng(1), 1).astype(np.float32)
    t = (0.1 * np.random.default_rng(1).normal(size=(1, 3))).astype(np.float32)
    g = np.asfortranarray(rng.standard_normal(size=(n, n, n, 1), dtype=np.float32))
    ref32 = oracle.raster((n,) * 3, pts, R, t, dtype=np.float32)
    ref64 = oracle.raster((n,) * 3, pts, R, t, dtype=np.float64)
    out = dpr_amd.raster((n,) * 3, T(pts, dev), T(R[0], dev), T(t[0], dev))  # algo="auto"
    o = out.cpu().numpy()
    assert_close(o, ref32[..., 0], tol(np.float32, "out"), "out vs fp32 oracle")
    assert_close(o, ref64[..., 0].astype(np.float32), 5e-5, "out vs fp64 oracle")
    rpb = oracle.raster_pullback(g, pts, R, t, dtype=np.float32)
    pb = dpr_amd.raster_pullback_(grid_to_dev(g[..., 0], dev), T(pts, dev), T(R[0], dev), T(t[0], dev))
    assert_close(pb.points, rpb.points, tol(np.float32, "points"), "ds_dpoints")
    assert_close(pb.rotation, rpb.rotation[0], tol(np.float32, "pose"), "ds_drotation")
    assert_close(pb.translation, rpb.translation[0], tol(np.float32, "pose"), "ds_dtranslation")
    report = {
        "config": "C2: 1M points -> 128^3 fp32, algo=auto (tiled)",
        "out_max_abs_err_vs_fp32_oracle": float(np.abs(o - ref32[..., 0]).max()),
        "out_max_abs_err_vs_fp64_oracle": float(np.abs(o - ref64[..., 0]).max()),
        "out_max_abs": float(np.abs(ref64).max()),
        "ds_dpoints_max_abs_err_vs_fp32_oracle": float(np.abs(pb.points.cpu().numpy() - rpb.points).max()),
        "cell_selection_flips_fp32_vs_fp64": _cell_flips(pts, R[0], t[0], n),
        "point_axis_pairs": 3 * P,
    }
    print("PARITY-REPORT " + json.dumps(report))
    outdir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(outdir) and os.access(outdir, os.W_OK):
        with open(os.path.join(outdir, "parity_report_c2.json"), "w") as f:
            json.dump(report, f, indent=1)


def test_c3_full_size_auto_vs_oracle_with_flip_report(oracle, dev):
    """BASELINE.json configs[2] at full size ON THE CLOUD bench.py TIMES (10 M points
    0.4*N(0,I) seed 0 in as-generated order, one random rotation, t = 0.1*N(0,I); 256^3, fp32),
    algo="auto" (the tiled pipeline), forward + pullback against the fp32 oracle and `out`
    against the fp64 oracle; SURVEY.md 8(c) report to gpurun_out/parity_report_c3.json."""
    import bench

    P, n = 10_000_000, 256
    assert dpr_amd.resolve_algo("raster", (n,) * 3, P, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (n,) * 3, P, 1, 3) == "tiled"
    pts = bench.synth_points("C3")
    R, t = bench.synth_poses("C3", 1, seed=1)
    assert pts.shape == (P, 3) and pts.dtype == np.float32
    g = np.asfortranarray(np.random.default_rng(2).standard_normal(size=(n, n, n, 1), dtype=np.float32))
    ref32 = oracle.raster((n,) * 3, pts, R, t, dtype=np.float32)
    ref64 = oracle.raster((n,) * 3, pts, R, t, dtype=np.float64)
    dp, dR, dt_ = T(pts, dev), T(R[0], dev), T(t[0], dev)
    out = dpr_amd.raster((n,) * 3, dp, dR, dt_)  # algo="auto"
    o = out.cpu().numpy()
    assert_close(o, ref32[..., 0], tol(np.float32, "out"), "out vs fp32 oracle")
    assert_close(o, ref64[..., 0].astype(np.float32), 5e-5, "out vs fp64 oracle")
    rpb = oracle.raster_pullback(g, pts, R, t, dtype=np.float32)
    pb = dpr_amd.raster_pullback_(grid_to_dev(g[..., 0], dev), dp, dR, dt_)
    assert_close(pb.points, rpb.points, tol(np.float32, "points"), "ds_dpoints")
    assert_close(pb.point_weight, rpb.point_weight, tol(np.float32, "points"), "ds_dpoint_weight")
    assert_close(pb.rotation, rpb.rotation[0], tol(np.float32, "pose"), "ds_drotation")
    assert_close(pb.translation, rpb.translation[0], tol(np.float32, "pose"), "ds_dtranslation")
    assert abs(float(pb.out_weight) - rpb.out_weight[0]) <= 1e-3 * abs(rpb.out_weight[0]) + 1e-3
    # the bench step's own pairing: forward keeps the binning, the pullback reuses it
    ws = torch.empty(dpr_amd.workspace_bytes("pullback", (n,) * 3, P, 1, 3, torch.float32, "tiled"),
                     dtype=torch.uint8, device=dev)
    out_k = dpr_amd.empty_grid((n,) * 3, None, torch.float32, dev)
    dpr_amd.raster_(out_k, dp, dR, dt_, algo="tiled", workspace=ws, keep_binning=True)
    pb_k = dpr_amd.raster_pullback_(grid_to_dev(g[..., 0], dev), dp, dR, dt_, algo="tiled",
                                    workspace=ws, reuse_binning=True)
    assert_close(out_k, ref32[..., 0], tol(np.float32, "out"), "out (keep) vs fp32 oracle")
    assert_close(pb_k.points, rpb.points, tol(np.float32, "points"), "ds_dpoints (reuse)")
    report = {
        "config": "C3: 10M points 0.4*N(0,I) seed 0, random order -> 256^3 fp32, algo=auto (tiled); "
                  "the cloud and pose bench.py times",
        "out_max_abs_err_vs_fp32_oracle": float(np.abs(o - ref32[..., 0]).max()),
        "out_max_abs_err_vs_fp64_oracle": float(np.abs(o - ref64[..., 0]).max()),
        "out_max_abs": float(np.abs(ref64).max()),
        "out_rel_l2_err_vs_fp64_oracle": float(np.linalg.norm((o - ref64[..., 0]).ravel())
                                               / np.linalg.norm(ref64.ravel())),
        "ds_dpoints_max_abs_err_vs_fp32_oracle": float(np.abs(pb.points.cpu().numpy() - rpb.points).max()),
        "ds_dpoints_equal_bit_for_bit": bool(np.array_equal(pb.points.cpu().numpy(), rpb.points)),
        "ds_drotation_rel_err": float(np.linalg.norm(pb.rotation.cpu().numpy() - rpb.rotation[0])
                                      / np.linalg.norm(rpb.rotation[0])),
        "cell_selection_flips_fp32_vs_fp64": _cell_flips(pts, R[0], t[0], n),
        "point_axis_pairs": 3 * P,
    }
    print("PARITY-REPORT " + json.dumps(report))
    outdir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(outdir) and os.access(outdir, os.W_OK):
        with open(os.path.join(outdir, "parity_report_c3.json"), "w") as f:
            json.dump(report, f, indent=1)


@pytest.mark.parametrize("algo", ["tiled", "atomic"])
def test_pose_offset_beyond_2_pow_32_elements(oracle, dev, algo):
    """Pose offsets b * G past 2^32 ELEMENTS: 33 poses of a 512^3 fp32 grid (17.7 GB per
    array, pose 32 starts at element 4.29e9).  The last pose against the single-pose oracle,
    forward and pullback (the other poses carry zero sensitivities, so the summed point
    gradients are the last pose's alone).  Guards the int64 pose strides of the kernels at the
    size of C5's one-GPU point (64 x 512^3)."""
    P, n, B = 100_000, 512, 33
    G = n ** 3
    assert (B - 1) * G >= 2 ** 32  # every element of the last pose lies at or past 2^32
    rng = np.random.default_rng(11)
    pts = (0.4 * rng.standard_normal(size=(P, 3))).astype(np.float32)
    R = D.random_rotations(rng, B).astype(np.float32)
    t = (0.1 * rng.normal(size=(B, 3))).astype(np.float32)
    ow = np.linspace(0.5, 1.5, B).astype(np.float32)
    bg = np.linspace(-1.0, 1.0, B).astype(np.float32)
    out = dpr_amd.raster((n,) * 3, T(pts, dev), T(R, dev), T(t, dev), T(bg, dev), T(ow, dev), algo=algo)
    last = B - 1
    ref = oracle.raster((n,) * 3, pts, R[last:], t[last:], bg[last:], ow[last:], dtype=np.float32)
    assert_close(out[..., last], ref[..., 0], tol(np.float32, "out"), "last pose of the batch")
    assert_close(out[..., 0], oracle.raster((n,) * 3, pts, R[:1], t[:1], bg[:1], ow[:1],
                                            dtype=np.float32)[..., 0], tol(np.float32, "out"), "pose 0")
    del out
    g = torch.zeros((B, n, n, n), dtype=torch.float32, device=dev)
    g_last = rng.standard_normal(size=(n, n, n, 1), dtype=np.float32)
    g[last] = torch.as_tensor(np.ascontiguousarray(np.transpose(g_last[..., 0], (2, 1, 0))), device=dev)
    pb = dpr_amd.raster_pullback_(g.permute(3, 2, 1, 0), T(pts, dev), T(R, dev), T(t, dev), T(bg, dev),
                                  T(ow, dev), algo=algo)
    rpb = oracle.raster_pullback(np.asfortranarray(g_last), pts, R[last:], t[last:], ow[last:],
                                 dtype=np.float32)
    assert_close(pb.points, rpb.points, tol(np.float32, "points"), "ds_dpoints")
    assert_close(pb.rotation[last], rpb.rotation[0], tol(np.float32, "pose"), "ds_drotation[last]")
    assert_close(pb.translation[last], rpb.translation[0], tol(np.float32, "pose"), "ds_dtranslation[last]")
    assert abs(float(pb.background[last]) - rpb.background[0]) <= 1e-3 * abs(rpb.background[0]) + 1e-2
    assert abs(float(pb.out_weight[last]) - rpb.out_weight[0]) <= 1e-3 * abs(rpb.out_weight[0]) + 1e-3
    assert float(pb.rotation[:last].abs().max()) == 0.0 and float(pb.background[:last].abs().max()) == 0.0


def test_chunk_owner_with_more_than_65535_poses(oracle, dev):
    """Every launch of the chunk-owner path that puts poses on grid.y is cut into blocks of at
    most 65535 (round-2 advisor finding: k_co_reduce was not).  65 600 poses of a small cloud
    on a 16 x 16 image; poses past the first launch block against the oracle."""
    P, n, B = 300, 16, 65_600
    rng = np.random.default_rng(3)
    pts = (0.4 * rng.standard_normal(size=(P, 3))).astype(np.float32)
    R = D.random_rotations(rng, B)[:, :2, :].astype(np.float32)
    t = (0.1 * rng.normal(size=(B, 2))).astype(np.float32)
    out = dpr_amd.raster((n, n), T(pts, dev), T(R, dev), T(t, dev), algo="chunked")
    g = torch.randn((B, n, n), dtype=torch.float32, device=dev)
    pb = dpr_amd.raster_pullback_(g.permute(2, 1, 0), T(pts, dev), T(R, dev), T(t, dev), algo="chunked")
    pa = dpr_amd.raster_pullback_(g.permute(2, 1, 0), T(pts, dev), T(R, dev), T(t, dev), algo="atomic")
    assert_close(pb.points, pa.points.cpu().numpy(), 1e-4, "ds_dpoints vs the direct kernels")
    sel = [0, 65_534, 65_535, 65_536, B - 1]
    ref = oracle.raster((n, n), pts, R[sel], t[sel], dtype=np.float32)
    gs = np.asfortranarray(np.transpose(g[sel].cpu().numpy(), (2, 1, 0)))
    rpb = oracle.raster_pullback(gs, pts, R[sel], t[sel], dtype=np.float32)
    for k, b in enumerate(sel):
        assert_close(out[..., b], ref[..., k], tol(np.float32, "out"), f"out pose {b}")
        assert_close(pb.rotation[b], rpb.rotation[k], tol(np.float32, "pose"), f"ds_drotation {b}")
        assert_close(pb.translation[b], rpb.translation[k], tol(np.float32, "pose"), f"ds_dtranslation {b}")
        assert abs(float(pb.out_weight[b]) - rpb.out_weight[k]) <= 1e-3 * abs(rpb.out_weight[k]) + 1e-4


# ------------------------------------------------------------------ the plain C entry points
def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("suf,npdt,tdt", [("f32", np.float32, torch.float32),
                                          ("f64", np.float64, torch.float64)])
def test_plain_entry_points_as_integration_md_binds_them(oracle, dev, suf, npdt, tdt):
    """dpr_raster_<T>, dpr_raster_pullback_<T> and dpr_raster_residual_pullback_<T> through raw
    ctypes with exactly the argument lists of INTEGRATION.md / the Julia extension's ccalls,
    workspace sized by dpr_workspace_bytes_<T>(op, algo=0, ...), P = 3e5 so that AUTO picks
    the tiled pipeline; results against the oracle."""
    L = dpr_amd.lib()
    P, n, B = 300_000, 96, 1
    d = D.make(n_points=P, n_in=3, n_out=3, batch=B, grid_n=n, seed=5, dtype=npdt)
    grid = np.array([n, n, n], dtype=np.int64)
    gp = grid.ctypes.data_as(ctypes.c_void_p)
    assert L.dpr_resolve_algo(dpr_amd._lib.OP_RASTER, 3, 3, gp, P, B) == dpr_amd._lib.ALGO_TILED
    wsq = getattr(L, f"dpr_workspace_bytes_{suf}")
    need = max(wsq(dpr_amd._lib.OP_RASTER, 0, 3, 3, gp, P, B),
               wsq(dpr_amd._lib.OP_PULLBACK, 0, 3, 3, gp, P, B))
    assert 0 < need < 1 << 32
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    pts = T(d.points, dev)
    rot_cm = T(np.ascontiguousarray(np.transpose(d.rotations, (0, 2, 1))), dev)  # col-major poses
    trans, bg, ow, pw = T(d.translations, dev), T(d.backgrounds, dev), T(d.weights, dev), T(d.point_weights, dev)
    out = torch.full((B, n, n, n), float("nan"), dtype=tdt, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = getattr(L, f"dpr_raster_{suf}")(stream, 3, 3, gp, P, B, _vp(out), _vp(pts), _vp(rot_cm),
                                         _vp(trans), _vp(bg), _vp(ow), _vp(pw), _vp(ws), need)
    assert rc == 0, dpr_amd._lib.last_error()
    ref = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                        d.point_weights, dtype=npdt)
    assert_close(out.permute(3, 2, 1, 0), ref, tol(npdt, "out"), "dpr_raster out")
    g = torch.as_tensor(np.ascontiguousarray(np.transpose(d.ds_dout, (3, 2, 1, 0))), device=dev)
    outs = [torch.full(s, float("nan"), dtype=tdt, device=dev)
            for s in [(P, 3), (B, 3, 3), (B, 3), (B,), (B,), (P,)]]
    rc = getattr(L, f"dpr_raster_pullback_{suf}")(
        stream, 3, 3, gp, P, B, _vp(g), _vp(pts), _vp(rot_cm), _vp(trans), _vp(ow), _vp(pw),
        *[_vp(o) for o in outs], _vp(ws), need)
    assert rc == 0, dpr_amd._lib.last_error()
    rpb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights,
                                 d.point_weights, dtype=npdt)
    assert_close(outs[0], rpb.points, tol(npdt, "points"), "ds_dpoints")
    assert_close(outs[1].transpose(1, 2), rpb.rotation, tol(npdt, "pose"), "ds_drotation")
    assert_close(outs[2], rpb.translation, tol(npdt, "pose"), "ds_dtranslation")
    assert_close(outs[3], rpb.background, tol(npdt, "pose"), "ds_dbackground")
    assert_close(outs[4], rpb.out_weight, tol(npdt, "pose"), "ds_dout_weight")
    assert_close(outs[5], rpb.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
    # residual form: out, target, scale ... loss, six outputs
    target = torch.as_tensor(np.ascontiguousarray(np.transpose(d.ds_dout, (3, 2, 1, 0))), device=dev)
    loss = torch.full((B,), float("nan"), dtype=tdt, device=dev)
    outs2 = [torch.full_like(o, float("nan")) for o in outs]
    rc = getattr(L, f"dpr_raster_residual_pullback_{suf}")(
        stream, 3, 3, gp, P, B, _vp(out), _vp(target), ctypes.c_double(2.0), _vp(pts), _vp(rot_cm),
        _vp(trans), _vp(ow), _vp(pw), _vp(loss), *[_vp(o) for o in outs2], _vp(ws), need)
    assert rc == 0, dpr_amd._lib.last_error()
    res, ref_loss = oracle.residual_pullback(ref, d.ds_dout, d.points, d.rotations, d.translations,
                                             d.weights, d.point_weights, scale=2.0, dtype=npdt)
    assert_close(outs2[0], res.points, 10 * tol(npdt, "points"), "residual ds_dpoints")
    assert_close(loss, ref_loss.astype(npdt), 1e-4 if npdt == np.float32 else 1e-10, "loss")


# ------------------------------------------------------------------ sharded drivers over RCCL
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture()
def nccl_world1(dev):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        yield dist
    finally:
        dist.destroy_process_group()


def test_pose_and_point_sharded_drivers_with_hip_compute_over_nccl(oracle, dev, nccl_world1):
    """`raster_sharded` / `raster_pullback_sharded_` and the point-sharded pair with their
    default (HIP) local compute inside an RCCL process group of one rank: the kernels libdpr
    enqueues on torch's stream feed the fused buffer / the grid straight into
    `dist.all_reduce` (which runs on RCCL's own stream).  Compared with the oracle."""
    npdt = np.float32
    d = D.make(n_points=400_000, n_in=3, n_out=3, batch=3, grid_n=64, seed=9, dtype=npdt)
    pts, Rs, ts = T(d.points, dev), T(d.rotations, dev), T(d.translations, dev)
    bgs, ows, pw = T(d.backgrounds, dev), T(d.weights, dev), T(d.point_weights, dev)
    out_local, (lo, hi) = dpr_amd.raster_sharded(d.grid, pts, Rs, ts, bgs, ows, pw)
    assert (lo, hi) == (0, 3)
    ref = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights,
                        d.point_weights, dtype=npdt)
    assert_close(out_local, ref, tol(npdt, "out"), "raster_sharded out")
    g = grid_to_dev(d.ds_dout, dev)
    fused = torch.full((d.n_points * 4,), float("nan"), dtype=torch.float32, device=dev)
    res = dpr_amd.raster_pullback_sharded_(g, pts, Rs, ts, bgs, ows, pw, fused_buffer=fused)
    rpb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights,
                                 d.point_weights, dtype=npdt)
    torch.cuda.synchronize()
    assert res.points.data_ptr() == fused.data_ptr()
    _compare(ref, rpb, out_local, res, npdt)
    # point sharding (single-pose style problems): grid all-reduce forward, scalars backward
    out2 = dpr_amd.raster_point_sharded(d.grid, pts, Rs, ts, bgs, ows, pw)
    assert_close(out2, ref, tol(npdt, "out"), "raster_point_sharded out")
    res2 = dpr_amd.raster_pullback_point_sharded_(g, pts, Rs, ts, bgs, ows, pw)
    _compare(ref, rpb, out2, res2, npdt)


@pytest.mark.parametrize("suf,npdt,tdt", [("f32", np.float32, torch.float32),
                                          ("f64", np.float64, torch.float64)])
@pytest.mark.parametrize("fused", [True, False])
def test_c_abi_sharded_pullback_over_rccl(oracle, dev, suf, npdt, tdt, fused):
    """dpr_comm_unique_id / dpr_comm_init / dpr_raster_pullback_sharded_<T> / dpr_comm_destroy
    through raw ctypes (what a non-Python host binds): a one-rank RCCL
    communicator on this GPU, the rank's pose block from dpr_shard_range, the all-reduce on the
    caller's stream.  Results against the oracle."""
    L = dpr_amd.lib()
    uid = (ctypes.c_char * 128)()
    assert L.dpr_comm_unique_id(uid, 128) == 0, dpr_amd._lib.last_error()
    comm = ctypes.c_void_p()
    with torch.cuda.device(dev):
        assert L.dpr_comm_init(ctypes.byref(comm), 1, 0, uid) == 0, dpr_amd._lib.last_error()
    try:
        assert L.dpr_comm_world(comm) == 1 and L.dpr_comm_rank(comm) == 0
        P, n, B = 300_000, 64, 5
        d = D.make(n_points=P, n_in=3, n_out=3, batch=B, grid_n=n, seed=13, dtype=npdt)
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        L.dpr_shard_range(B, 0, 1, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == (0, B)
        grid = np.array([n, n, n], dtype=np.int64)
        gp = grid.ctypes.data_as(ctypes.c_void_p)
        need = getattr(L, f"dpr_workspace_bytes_{suf}")(dpr_amd._lib.OP_PULLBACK, 0, 3, 3, gp, P, B)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        pts = T(d.points, dev)
        rot_cm = T(np.ascontiguousarray(np.transpose(d.rotations, (0, 2, 1))), dev)
        trans, ow, pw = T(d.translations, dev), T(d.weights, dev), T(d.point_weights, dev)
        g = torch.as_tensor(np.ascontiguousarray(np.transpose(d.ds_dout, (3, 2, 1, 0))), device=dev)
        buf = torch.full((P * 4 + 64,), float("nan"), dtype=tdt, device=dev)
        d_pts = buf[: P * 3].view(P, 3)
        d_pw = buf[P * 3: P * 4] if fused else buf[P * 3 + 64:]
        outs = [torch.full(s, float("nan"), dtype=tdt, device=dev) for s in [(B, 3, 3), (B, 3), (B,), (B,)]]
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = getattr(L, f"dpr_raster_pullback_sharded_{suf}")(
            comm, stream, 3, 3, gp, P, B, _vp(g), _vp(pts), _vp(rot_cm), _vp(trans), _vp(ow), _vp(pw),
            _vp(d_pts), *[_vp(o) for o in outs], _vp(d_pw), _vp(ws), ws.numel())
        assert rc == 0, dpr_amd._lib.last_error()
        torch.cuda.synchronize()
        rpb = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights,
                                     d.point_weights, dtype=npdt)
        assert_close(d_pts, rpb.points, tol(npdt, "points"), "ds_dpoints")
        assert_close(d_pw, rpb.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
        assert_close(outs[0].transpose(1, 2), rpb.rotation, tol(npdt, "pose"), "ds_drotation")
        assert_close(outs[1], rpb.translation, tol(npdt, "pose"), "ds_dtranslation")
        assert_close(outs[2], rpb.background, tol(npdt, "pose"), "ds_dbackground")
        assert_close(outs[3], rpb.out_weight, tol(npdt, "pose"), "ds_dout_weight")
    finally:
        assert L.dpr_comm_destroy(comm) == 0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (one rank per GPU)")
def test_bench_two_ranks_over_rccl(tmp_path):
    """bench.py --gpus 2 from a bare shell: its own launcher, one rank per GPU, RCCL exchange."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--poses", "8",
                        "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0


def test_bench_pose_exchange_step_over_a_one_rank_rccl_group():
    """The exchange step every `bench.py --gpus N > 1` run executes -- pose block from
    shard_range, fused gradient buffer, double buffer, `dist.all_reduce(async_op=True)` over
    "nccl" (= RCCL), `pending[k].wait()` before the buffer is written again, drain before the
    closing barrier -- driven on ONE GPU with `--force-exchange` (a one-rank RCCL group).  The
    two-rank test above is skipped on every one-GPU box; this one is not."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C4",
                        "--poses", "6", "--force-exchange", "--steps", "3", "--warmup", "2",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["steps"] == 3
    ex = line["config"]["exchange"]
    assert "all-reduce(sum)" in ex and "(nccl)" in ex and "overlapped" in ex, ex
    # what the driver's SCALE record checks an N-rank run with: the ranks RCCL saw, and its version
    assert line["config"]["ranks_seen"] == 1
    assert str(line["config"]["rccl_version"])[0].isdigit(), line["config"]["rccl_version"]
    # and serialised (no double buffer): the all-reduce completes inside each step
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C4",
                         "--poses", "6", "--force-exchange", "--no-overlap-exchange", "--steps", "2",
                         "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "inside the step" in json.loads(r2.stdout.strip().splitlines()[-1])["config"]["exchange"]


def test_bench_default_line_carries_the_scaling_reference():
    """`bench.py` at --gpus 1 keeps C3 as the headline and adds `scaling_reference`: the job of
    the N > 1 runs (C4, 512 poses) on one GPU, so that a 1 -> N curve compares one job."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-secondary"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["config"]["workload"].startswith("C3") and line["scaling"] == "weak"
    ref = line["scaling_reference"]
    assert ref["poses_global"] == 512 and ref["value"] > 0 and ref["ms_per_step"] > 0
    assert ref["algo"]["raster"] == "chunked"
    assert line["roofline"]["frac"] > 0 and line["roofline"]["ms"] > 0
    # the ceiling of the 8-GPU curve from one-GPU measurements, and both step figures of the headline
    assert ref["share_of_one_gpu_of_8"]["poses"] == 64 and ref["share_of_one_gpu_of_8"]["ms_per_step"] > 0
    assert 1.0 < ref["predicted_speedup_at_8_gpus_before_exchange"] <= 8.5
    assert line["ms_per_step_cold"] > 0 and len(line["ms_per_step_loops"]) == 3
    assert isinstance(line["config"]["untimed_steps"], int) and line["config"]["untimed_steps"] >= 3 + 1 + 2


def test_bench_dump_outputs_are_the_step_outputs_and_repeat(oracle, dev, tmp_path):
    """`bench.py --dump-outputs DIR`: the last timed step's forward grid and pullback gradients as .npy
    files; two runs with the same arguments see the same inputs (C1: against the oracle as well)."""
    import subprocess
    import sys

    import bench

    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C1", "--steps", "2",
                            "--warmup", "1", "--loops", "1", "--no-spin-up", "--no-cpu-baseline",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        assert sorted(line["dumped_outputs"]["arrays"]) == sorted(
            ["out", "ds_dpoints", "ds_drotation", "ds_dtranslation", "ds_dbackground", "ds_dout_weight",
             "ds_dpoint_weight"])
        dumps.append({n: np.load(d / f"{n}.npy") for n in line["dumped_outputs"]["arrays"]})
    for n, a in dumps[0].items():
        assert a.dtype == np.float64, n
        assert_close(dumps[1][n], a, 1e-12)  # (atomics: equal up to the summation order)
    # what the step computed: C1's seeded inputs through the oracle
    pts = bench.synth_points("C1")
    R, t = bench.synth_poses("C1", 1, seed=1)
    ref = oracle.raster((5, 5), pts, R, t)
    assert_close(dumps[0]["out"], ref[..., 0], 1e-12, "out")
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)  # bench.py's ds_dout of rank 0: randn of the reversed grid shape, seen [i1, i2]
    g = torch.randn((5, 5), device=dev, dtype=torch.float64, generator=gen).permute(1, 0).cpu().numpy()
    rpb = oracle.raster_pullback(g[..., None], pts, R, t)
    for n, e in (("ds_dpoints", rpb.points), ("ds_drotation", rpb.rotation[0]),
                 ("ds_dtranslation", rpb.translation[0]), ("ds_dbackground", rpb.background[0]),
                 ("ds_dout_weight", rpb.out_weight[0]), ("ds_dpoint_weight", rpb.point_weight)):
        assert_close(dumps[0][n], e, 1e-10, n)


# ------------------------------------------------------------------ the FULL jobs, checked once
def test_c4_full_job_512_poses_against_the_oracle(oracle, dev):
    """BASELINE.json configs[3] as ONE GPU runs it for the N > 1 curve's one-GPU point
    (`scaling_reference` of bench.py): 10 M points -> 512^2, ALL 512 poses, fp32, AUTO (the
    chunk-owner path in pose slices of 64).  Three poses -- the first, the first of the second
    slice, the last -- against single-pose oracle calls on the whole cloud, forward and per-pose
    gradients; the point gradients (sums over all 512 poses) against the batched oracle on a
    10^5-point subsample of the cloud (a point's gradient depends on no other point)."""
    import bench

    P, n, B = 10_000_000, 512, 512
    assert dpr_amd.resolve_algo("raster", (n, n), P, B, 3) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (n, n), P, B, 3) == "chunked"
    np_pts = bench.synth_points("C4")
    np_R, np_t = bench.synth_poses("C4", B, seed=1)
    pts, R, t = T(np_pts, dev), T(np_R, dev), T(np_t, dev)
    rng = np.random.default_rng(11)
    np_ow = rng.uniform(0.5, 2.0, B).astype(np.float32)
    ow = T(np_ow, dev)
    check = [0, 64, B - 1]
    out = dpr_amd.raster((n, n), pts, R, t, None, ow)
    g = torch.randn(B, n, n, device=dev, dtype=torch.float32,
                    generator=torch.Generator(device=dev).manual_seed(2)).permute(2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, pts, R, t, None, ow)
    np_g = g.cpu().numpy()  # [i1, i2, b]
    for b in check:
        ref = oracle.raster((n, n), np_pts, np_R[b:b + 1], np_t[b:b + 1], None, np_ow[b:b + 1],
                            dtype=np.float32)
        assert_close(out[..., b], ref[..., 0], 5e-5, f"out, pose {b}")
        # the fp32 oracle: identical arithmetic per contribution, hence identical cell choice (against
        # fp64 arithmetic ~2000 of the 10^7 points sit within rounding of a cell boundary and pick
        # the other cell, where the gradient of the piecewise-bilinear interpolant is another one:
        # 1 % of these sums -- SURVEY.md section 7, "cell-selection discontinuity")
        rp = oracle.raster_pullback(np_g[..., b:b + 1], np_pts, np_R[b:b + 1], np_t[b:b + 1],
                                    np_ow[b:b + 1], dtype=np.float32)
        assert_close(pb.rotation[b], rp.rotation[0], 1e-3, f"ds_drotation, pose {b}")
        assert_close(pb.translation[b], rp.translation[0], 1e-3, f"ds_dtranslation, pose {b}")
        assert abs(float(pb.out_weight[b]) - rp.out_weight[0]) <= 1e-3 * max(abs(rp.out_weight[0]), np.sqrt(P))
        assert abs(float(pb.background[b]) - rp.background[0]) <= 1e-3 * n
    sub = rng.choice(P, 100_000, replace=False)
    rs = oracle.raster_pullback(np_g, np_pts[sub], np_R, np_t, np_ow, dtype=np.float32, threaded=True)
    assert_close(pb.points[T(sub, dev)], rs.points, 1e-4, "ds_dpoints of the subsample (512 poses summed)")
    assert_close(pb.point_weight[T(sub, dev)], rs.point_weight, 1e-4, "ds_dpoint_weight of the subsample")


def test_c5_full_batch_64_poses_against_the_oracle(oracle, dev):
    """BASELINE.json configs[4] with its FULL batch on one GPU: 64 poses of a 512^3 fp64 grid
    (68.7 GB each for `out` and `ds_dout`), AUTO -> the tiled path with the cloud cell-sorted
    inside the call and the poses binned in batches of 8.  The cloud is a 5 M-point subsample of
    the config's 50 M (the grids are what is large here; the share of one GPU of 8 runs the full
    cloud in test_c5_share_8_poses).  Three poses -- the first, the first of the second batch,
    the last -- against single-pose oracle calls, forward and pullback; `ds_dout` is non-zero
    on those three poses only, so the summed point gradients are the oracle's over three poses."""
    import bench

    P, n, B = 5_000_000, 512, 64
    # (5 M points are SPARSE on 512^3 -- one per 27 voxels: since round 5 AUTO sorts such a batch inside the call
    # and runs the chunk lists; the config's own 50 M points stay on the tiled path)
    assert dpr_amd.resolve_algo("raster", (n, n, n), P, B, 3) == "chunked"
    assert dpr_amd.resolve_algo("raster", (n, n, n), 50_000_000, B, 3) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (n, n, n), P, B, 3) == "chunked"
    np_pts = bench.synth_points("C5")[:P]
    np_R, np_t = bench.synth_poses("C5", B, seed=1)
    pts, R, t = T(np_pts, dev), T(np_R, dev), T(np_t, dev)
    check = [0, 8, B - 1]
    out = dpr_amd.raster((n, n, n), pts, R, t)
    for b in check:
        ref = oracle.raster((n, n, n), np_pts, np_R[b:b + 1], np_t[b:b + 1], threaded=True)
        assert_close(out[..., b], ref[..., 0], 1e-10, f"out, pose {b}")
        del ref
    mass = out.sum(dim=(0, 1, 2)).cpu().numpy()
    in_grid = float(out[..., 0].sum())
    np.testing.assert_allclose(mass, np.full(B, in_grid), rtol=0.1)  # (every pose holds about the same mass)
    del out
    torch.cuda.empty_cache()
    g = torch.zeros(B, n, n, n, device=dev, dtype=torch.float64)
    gen = torch.Generator(device=dev).manual_seed(4)
    for b in check:
        g[b].normal_(generator=gen)
    g = g.permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, pts, R, t)
    np_g = np.asfortranarray(np.stack([g[..., b].cpu().numpy() for b in check], axis=-1))
    rp = oracle.raster_pullback(np_g, np_pts, np_R[check], np_t[check], threaded=True)
    assert_close(pb.points, rp.points, 1e-10, "ds_dpoints (three poses carry sensitivity)")
    assert_close(pb.point_weight, rp.point_weight, 1e-10, "ds_dpoint_weight")
    for k, b in enumerate(check):
        assert_close(pb.rotation[b], rp.rotation[k], 1e-9, f"ds_drotation, pose {b}")
        assert_close(pb.translation[b], rp.translation[k], 1e-9, f"ds_dtranslation, pose {b}")
        assert abs(float(pb.out_weight[b]) - rp.out_weight[k]) <= 1e-9 * max(abs(rp.out_weight[k]), 1.0)
        assert abs(float(pb.background[b]) - rp.background[k]) <= 1e-8 * float(np.abs(np_g[..., k]).sum())
    others = [b for b in range(B) if b not in check]
    assert float(pb.rotation[others].abs().max()) == 0.0 and float(pb.out_weight[others].abs().max()) == 0.0


@pytest.mark.parametrize("npdt,tdt,batch,share", [(np.float64, torch.float64, 11, False),
                                                  (np.float32, torch.float32, 19, True)])
def test_local_batches_with_a_remainder(oracle, dev, npdt, tdt, batch, share):
    """Local binning bins up to 8 poses per launch (all B poses, 16 per launch, for a kept batch):
    11 poses = a batch of 8 + one of 3, 19 kept poses = 16 + 3 -- on a grid of 4100 tiles, where the
    cloud is cell-sorted inside the call (fp64: the 512-thread direct-store binning).  Forward and
    pullback (re-binning, or reusing the kept binning) against the oracle, with point weights."""
    grid = (320, 320, 328)  # 5 x 20 x 41 tiles
    d = D.make(n_points=220_000, n_in=3, n_out=3, batch=batch, grid_n=grid, seed=41, dtype=npdt)
    args = (T(d.points, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev),
            T(d.weights, dev), T(d.point_weights, dev))
    ws = None
    if share:
        need = max(dpr_amd.workspace_bytes(op, d.grid, d.n_points, batch, 3, tdt, "tiled", sharing=True)
                   for op in ("raster", "pullback"))
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, batch, tdt, dev)
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=share)
    # four poses against the single-pose oracle: first / last of the first launch, first of the
    # second, the last
    for b in sorted({0, 7, 8, batch - 1}):
        ref = oracle.raster(d.grid, d.points, d.rotations[b:b + 1], d.translations[b:b + 1],
                            d.backgrounds[b:b + 1], d.weights[b:b + 1], d.point_weights, dtype=npdt)
        assert_close(out[..., b], ref[..., 0], tol(npdt, "out"), f"out, pose {b}")
    del out
    # sensitivities on three poses only (first of a launch, last of the first launch, last pose)
    hot = [0, 7, batch - 1]
    g = torch.zeros((batch,) + tuple(reversed(grid)), device=dev, dtype=tdt)
    gen = torch.Generator(device=dev).manual_seed(9)
    for b in hot:
        g[b].normal_(generator=gen)
    g = g.permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, *args, algo="tiled", workspace=ws, reuse_binning=share)
    np_g = np.asfortranarray(np.stack([g[..., b].cpu().numpy() for b in hot], axis=-1))
    rp = oracle.raster_pullback(np_g, d.points, d.rotations[hot], d.translations[hot], d.weights[hot],
                                d.point_weights, dtype=npdt)
    assert_close(pb.points, rp.points, tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight, rp.point_weight, tol(npdt, "points"), "ds_dpoint_weight")
    for k, b in enumerate(hot):
        assert_close(pb.rotation[b], rp.rotation[k], tol(npdt, "pose"), f"ds_drotation, pose {b}")
        assert_close(pb.translation[b], rp.translation[k], tol(npdt, "pose"), f"ds_dtranslation, pose {b}")
    cold = [b for b in range(batch) if b not in hot]
    assert float(pb.rotation[cold].abs().max()) == 0.0
