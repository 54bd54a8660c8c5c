"""The prologues of the REUSE pullback on DPR_ALGO_TILED: k_tile_gather / k_tile_gather_runs request their work
item, the item count, the pose and the words of the binning header in one batch and form the verdict afterwards;
k_unpermute_runs / k_unpermute request their map entries before they look at the verdict.  Loads first, verdict
after, nothing stored before it -- so three things are held here:

  1. same results: a KEEP forward + REUSE pullback gives the bytes of the plain pullback in ds_dpoints,
     ds_dpoint_weight and ds_dbackground (one pose: the same binning, one gradient record per point, f64 sums of
     the staged ds_dout in a fixed order), and the three per-pose sums at the tolerance tests/test_parity_gpu.py
     holds the tiled pullback to (their order inside a tile varies run to run);
  2. the verdict still guards every output: REUSE on a workspace no KEEP forward wrote, or one written for another
     pose, another P or another points tensor, or one filled with 0xFF bytes, returns NaN everywhere and touches
     nothing outside the outputs and the workspace (4 KiB guard bands on both sides of each);
  3. dropped points and empty tiles: exact zeros for the points outside the grid, the plain pullback's bytes for
     the others.

Regimes (the smallest at which these paths differ): 128 x 32 x 16 = 8 tiles of 64 x 16 x 8 with 5 000 Gaussian
points, fp32 and fp64; the same with 20 000 more points inside one tile, which is then split into parts
(`first_part`, the parts' partials); 64 x 64 = 4 tiles of 32 x 32 with 3 000 points; local binning
(coherent_points=True: k_tile_gather_runs); four poses (k_unpermute: a pose group in the plain pullback, the kept
per-pose binnings summed in one pass in the REUSE one).  For the four poses the plain and the REUSE pullback group
the poses differently (include/dpr.h, SUMMATION ORDER: "added per point in a fixed order, group by group"), so
there the point gradients and ds_dbackground are held to the parity tolerances instead of ==.
"""
import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests.test_parity_gpu import T, assert_close, grid_to_dev, tol

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
F32, F64 = (np.float32, torch.float32), (np.float64, torch.float64)
G3, G2 = (128, 32, 16), (64, 64)
TILE = {3: (64, 16, 8), 2: (32, 32)}
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")

# name -> (n_out, grid, P, poses, heavy tile, keyword arguments of both calls)
REGIMES = {
    "3d": (3, G3, 5000, 1, False, {}),
    "3d-heavy": (3, G3, 5000, 1, True, {}),
    "2d": (2, G2, 3000, 1, False, {}),
    "3d-local": (3, G3, 5000, 1, False, dict(coherent_points=True)),
    "3d-group": (3, G3, 5000, 4, False, {}),
}
SAME = [(r, dt) for r in REGIMES for dt in (F32, F64)]
VERDICT = [("3d", F32), ("3d", F64), ("3d-heavy", F32), ("2d", F32), ("3d-local", F32), ("3d-group", F32)]
ids = lambda cases: [f"{r}-{np.dtype(dt[0]).name}" for r, dt in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def same_bytes(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def points_at(d, voxel, b=0):
    """Points whose projection under pose b has the voxel coordinates `voxel` (coord of dpr_device.h,
    ref_and_deltas: (R p + t + 1) n / 2; the rotations of tests/data.py are orthogonal 3 x 3 blocks, so for
    n_out = 2 the missing coordinate is set to 0)."""
    n = np.asarray(d.grid, dtype=np.float64)
    proj = voxel * (2.0 / n) - 1.0 - d.translations[b].astype(np.float64)
    R = d.rotations[b].astype(np.float64)  # (n_out, n_in), rows of an orthogonal matrix
    return proj @ R


def make(regime, npdt, seed=0):
    n_out, grid, P, B, heavy, kw = REGIMES[regime]
    d = D.make(n_points=P, n_in=3, n_out=n_out, batch=B, grid_n=grid, seed=40 + seed, dtype=npdt)
    if heavy:
        # 20 000 more points well inside tile (1, 0, 1): far above the split threshold of 4096 records
        rng = np.random.default_rng(5 + seed)
        t = np.asarray(TILE[n_out], dtype=np.float64)
        lo = np.array([1, 0, 1], dtype=np.float64) * t
        voxel = lo + 1.0 + rng.uniform(size=(20_000, n_out)) * (t - 2.0)
        d.points = np.ascontiguousarray(np.concatenate([d.points, points_at(d, voxel)]), dtype=npdt)
        pw = rng.uniform(0.5, 1.5, size=d.points.shape[0])
        d.point_weights = np.ascontiguousarray(pw / pw.sum(), dtype=npdt)
        d.n_points = d.points.shape[0]
    return d, kw


def dev_args(d, dev):
    return [T(d.points, dev), T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev), T(d.weights, dev),
            T(d.point_weights, dev)]


def workspace_need(d, tdt, kw, n_points=None):
    return max(dpr_amd.workspace_bytes(op, d.grid, n_points or d.n_points, d.batch, d.n_in, tdt, "tiled",
                                       sharing=True, **kw) for op in ("raster", "pullback"))


def keep_reuse(d, dev, tdt, args, g, kw, ws=None):
    if ws is None:
        ws = torch.empty(workspace_need(d, tdt, kw), dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, d.batch, tdt, dev)
    dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True, **kw)
    return dpr_amd.raster_pullback_(g, *args, algo="tiled", workspace=ws, reuse_binning=True, **kw)


def assert_same_results(pb_r, pb, npdt, exact):
    if exact:
        assert same_bytes(pb_r.points, pb.points), "ds_dpoints: KEEP / REUSE against the plain pullback"
        assert same_bytes(pb_r.point_weight, pb.point_weight), "ds_dpoint_weight: KEEP / REUSE against plain"
        assert same_bytes(pb_r.background, pb.background), "ds_dbackground: KEEP / REUSE against plain"
    else:
        assert_close(pb_r.points, pb.points.cpu().numpy(), tol(npdt, "points"), "ds_dpoints")
        assert_close(pb_r.point_weight, pb.point_weight.cpu().numpy(), tol(npdt, "points"), "ds_dpoint_weight")
        assert_close(pb_r.background, pb.background.cpu().numpy(), tol(npdt, "pose"), "ds_dbackground")
    assert_close(pb_r.rotation, pb.rotation.cpu().numpy(), tol(npdt, "pose"), "ds_drotation")
    assert_close(pb_r.translation, pb.translation.cpu().numpy(), tol(npdt, "pose"), "ds_dtranslation")
    assert_close(pb_r.out_weight, pb.out_weight.cpu().numpy(), tol(npdt, "pose"), "ds_dout_weight")


# ------------------------------------------------------------------ 1. same results
@pytest.mark.parametrize("regime,dt", SAME, ids=ids(SAME))
def test_keep_reuse_equals_the_plain_pullback(oracle, dev, regime, dt):
    npdt, tdt = dt
    d, kw = make(regime, npdt)
    args, g = dev_args(d, dev), grid_to_dev(d.ds_dout, dev)
    pb = dpr_amd.raster_pullback_(g, *args, algo="tiled", **kw)
    ref = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, d.point_weights,
                                 dtype=npdt)
    for name in FIELDS:
        kind = "points" if name in ("points", "point_weight") else "pose"
        assert_close(getattr(pb, name), getattr(ref, name), tol(npdt, kind), f"plain pullback, ds_d{name}")
    pb_r = keep_reuse(d, dev, tdt, args, g, kw)
    assert_same_results(pb_r, pb, npdt, exact=d.batch == 1)
    if d.batch > 1:
        # the pullback that bins pose by pose adds the poses as the kept binnings are added (held for the point
        # gradients by tests/test_sum_order_gpu.py::test_tiled_pullback_on_a_kept_binning), and sums the same
        # per-tile partials of ds_dout per pose in the same order
        pb_1 = dpr_amd.raster_pullback_(g, *args, algo="tiled", max_pose_group=1, **kw)
        assert_same_results(pb_r, pb_1, npdt, exact=True)


# ------------------------------------------------------------------ 2. the verdict guards every output
def guarded(nbytes, dev):
    """(whole buffer, interior view of `nbytes` bytes) with GUARD bytes of GUARD_BYTE on both sides"""
    buf = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def guarded_outputs(d, tdt, dev):
    """Pre-allocated outputs of raster_pullback_ inside guard bands, filled with 1 (finite: NaN has to be
    written); name -> (whole buffer, tensor)."""
    B, P, ni, no = d.batch, d.n_points, d.n_in, d.n_out
    shapes = dict(points=(P, ni), rotation=(B, ni, no), translation=(B, no), background=(B,), out_weight=(B,),
                  point_weight=(P,))
    esz = torch.empty((), dtype=tdt).element_size()
    out = {}
    for name, shape in shapes.items():
        buf, inner = guarded(int(np.prod(shape)) * esz, dev)
        t = inner.view(tdt).view(shape)
        t.fill_(1.0)
        out[name] = (buf, t.transpose(1, 2) if name == "rotation" else t)
    return out


def assert_guards(bufs, what):
    for name, buf in bufs.items():
        band = torch.full((GUARD,), GUARD_BYTE, dtype=torch.uint8, device=buf.device)
        assert torch.equal(buf[:GUARD], band), f"{what}: bytes in front of {name} were overwritten"
        assert torch.equal(buf[-GUARD:], band), f"{what}: bytes behind {name} were overwritten"


@pytest.mark.parametrize("regime,dt", VERDICT, ids=ids(VERDICT))
def test_reuse_without_its_forward_is_nan_and_stays_inside(dev, regime, dt):
    npdt, tdt = dt
    d, kw = make(regime, npdt)
    args, g = dev_args(d, dev), grid_to_dev(d.ds_dout, dev)
    need = workspace_need(d, tdt, kw)
    ws_buf, ws = guarded(need, dev)
    assert ws.data_ptr() % 256 == 0
    out_img = dpr_amd.empty_grid(d.grid, d.batch, tdt, dev)
    keep = lambda a, w=ws: dpr_amd.raster_(out_img, *a, algo="tiled", workspace=w, keep_binning=True, **kw)

    def reuse_is_nan(what, a=args):
        outs = guarded_outputs(d, tdt, dev)
        pb = dpr_amd.raster_pullback_(g, *a, algo="tiled", workspace=ws, reuse_binning=True,
                                      **{f"ds_d{k}": v[1] for k, v in outs.items()}, **kw)
        torch.cuda.synchronize()
        for name in FIELDS:
            got = getattr(pb, name)
            assert got.numel() == outs[name][1].numel()
            assert bool(torch.isnan(got).all()), f"{what}: ds_d{name} is not NaN everywhere"
            assert bool(torch.isnan(outs[name][1]).all()), f"{what}: the caller's ds_d{name} is not NaN everywhere"
        assert_guards(dict({k: v[0] for k, v in outs.items()}, workspace=ws_buf), what)

    # no KEEP forward ran on this workspace
    ws.zero_()
    reuse_is_nan("nothing kept")
    # ... it ran with another pose
    other_pose = list(args)
    other_pose[2] = args[2] + 0.01
    keep(other_pose)
    reuse_is_nan("kept for another pose")
    # ... with another P (the first P - 7 points of the same tensor: the same address)
    fewer = list(args)
    fewer[0], fewer[5] = args[0][:d.n_points - 7], args[5][:d.n_points - 7]
    assert fewer[0].data_ptr() == args[0].data_ptr()
    assert workspace_need(d, tdt, kw, d.n_points - 7) <= need
    keep(fewer)
    reuse_is_nan("kept for another P")
    # ... with another points tensor holding the same values
    clone = list(args)
    clone[0] = args[0].clone()
    keep(clone)
    reuse_is_nan("kept for another points tensor")
    # every byte of the workspace 0xFF: the largest count, the largest record range, NaN poses
    ws.fill_(0xFF)
    reuse_is_nan("workspace of 0xFF bytes")
    # and the pair itself still works on this workspace
    pb = dpr_amd.raster_pullback_(g, *args, algo="tiled", **kw)
    pb_r = keep_reuse(d, dev, tdt, args, g, kw, ws=ws)
    torch.cuda.synchronize()
    assert_same_results(pb_r, pb, npdt, exact=d.batch == 1)
    assert_guards(dict(workspace=ws_buf), "the matching pair")


# ------------------------------------------------------------------ 3. dropped points and empty tiles
DROPPED = [("3d", F32), ("3d", F64), ("2d", F32), ("3d-local", F32)]


@pytest.mark.parametrize("regime,dt", DROPPED, ids=ids(DROPPED))
def test_dropped_points_and_empty_tiles(dev, regime, dt):
    """Two thirds of the points are spread over the lower half of the grid along its last axis, at least 1.5 voxels
    below the first tile layer of the upper half (a record belongs to the tile of its LOWER neighbour: the upper
    tiles hold no record); every third point lies 10 units away from the grid."""
    npdt, tdt = dt
    d, kw = make(regime, npdt)
    P, n_out = d.n_points, d.n_out
    rng = np.random.default_rng(21)
    n = np.asarray(d.grid, dtype=np.float64)
    hi = n - 1.0
    hi[-1] = n[-1] / 2 - 1.5
    pts = points_at(d, 0.5 + rng.uniform(size=(P, n_out)) * (hi - 0.5))
    dropped = np.arange(P) % 3 == 2
    pts[dropped] += 10.0
    d.points = np.ascontiguousarray(pts, dtype=npdt)
    # what the construction is for, checked on the points as the library gets them (fp64 projection of the rounded
    # points; the margins of 1.5 voxels and 10 units dwarf the rounding): the dropped points miss the grid, the others
    # are inside, and the tiles that hold the others' records (tile of the lower neighbour, clamped at 0: DESIGN.md
    # 4.2) are a proper subset of the grid's tiles
    proj = d.points.astype(np.float64) @ d.rotations[0].astype(np.float64).T + d.translations[0].astype(np.float64)
    c = (proj + 1.0) * (n / 2.0) - 0.5
    outside = np.any((c <= -1.0) | (c > n), axis=1)
    assert outside[dropped].all() and not outside[~dropped].any()
    tile = np.asarray(TILE[n_out])
    lower = np.maximum(np.ceil(c[~dropped]).astype(np.int64) - 1, 0)
    used = {tuple(t) for t in lower // tile}
    n_tiles = int(np.prod(-(-np.asarray(d.grid) // tile)))
    assert 0 < len(used) < n_tiles, f"{len(used)} of {n_tiles} tiles hold a record: no empty tile"
    args, g = dev_args(d, dev), grid_to_dev(d.ds_dout, dev)
    pb = dpr_amd.raster_pullback_(g, *args, algo="tiled", **kw)
    pb_r = keep_reuse(d, dev, tdt, args, g, kw)
    assert_same_results(pb_r, pb, npdt, exact=True)
    r = torch.as_tensor(np.nonzero(dropped)[0], device=dev)
    kept = torch.as_tensor(np.nonzero(~dropped)[0], device=dev)
    for x in (pb, pb_r):
        assert not bool(x.points[r].abs().max() > 0), "dropped points: ds_dpoints"
        assert not bool(x.point_weight[r].abs().max() > 0), "dropped points: ds_dpoint_weight"
        # (the others do receive a gradient: ds_dout is Gaussian, no point weight is 0)
        assert bool((x.point_weight[kept] != 0).all()), "points inside the grid: ds_dpoint_weight"
