"""The launch cuts of the smooth rigid-body families at B = 65 600 images (past gridDim.y = 65535): P = 300, grid
(8, 8), K = 3 bodies with shuffled labels, pairs (2, 2) and (3, 2) -- the pattern of
test_smooth_poses_across_the_launch_cuts and test_sample_smooth_poses_across_the_launch_cuts of
tests/test_index_ranges_gpu.py.

  smooth_bodies_fwd_atomic, smooth_bodies_jvp_atomic   the images stride over gridDim.y = min(B, 65535)
  k_smooth_bodies_bwd, k_sample_smooth_bodies_fwd,     image slices from blockIdx.y (2 blocks of points: 1010 slices of
  k_sample_smooth_bodies_bwd                           65 images, the last of 15)
  smooth_bodies_bin_group, k_smooth_bodies_tile        nb * blocks_per_image and nb * tiles blocks for a group of
                                                       nb = 55 924 images, then a last group of 9 676 from b0 = 55 924

out_weight, ds_dout, the image and ds_dvalues are non-zero only in the images of `around_the_cut(B)` (0, 65534, 65535,
65536, 65599; the tiled case adds 55923, 55924, 55925), so the numpy references (tests/smooth_bodies_reference.py,
tests/smooth_bodies_jvp_reference.py, tests/sample_smooth_bodies_reference.py; fp64 on inputs rounded to fp32 once)
are evaluated on those images only and every other plane, column and per-(image, body) sum is exactly its background
or 0.  Pullback outputs are caller buffers pre-filled with NaN.  Tolerances: tol() of tests/test_parity_gpu.py, per
plane and per (image, body).

Mutation record: the seven mutants of tests/test_smooth_bodies_hard_gpu.py's docstring, each run once against this
module as well (every one keeps its accesses inside its buffers).  Failed here first:
  1 load_body_pose always scalar                   smooth_bodies_images_across_the_launch_cuts[2-2-float32]: out[.., 0],
                                                    26 % off
  2 k_smooth_bodies_keys: the tile from image b0   tiled_forward_groups_across_the_launch_cuts[2-2]: out[.., 55925],
                                                    0.8 % off -- an image of the second group whose points the pose of
                                                    image 55924 rejects (8 tests pass before)
  6 k_sample_smooth_bodies_bwd keeps `tab[i]`      sample_smooth_bodies_images_across_the_launch_cuts[2-2-float32]:
    after the flush                                 ds_drotation[65535, 0], 122 % off: the sums of image 65534 of the
                                                    same slice (the two hard modules pass: their slices hold one image)
  7 smooth_bodies_jvp_atomic's kernel stops at     smooth_bodies_jvp_images_across_the_launch_cuts[2-2-float32]:
    image min(B, 65535) (no stride)                 out_dot[.., 0, 65535], 101 % off
Mutants 3, 4 and 5 pass this module: one tile whose halo lies outside the grid, V = 1 on atomic only, and no tiled
sampling pullback at this B; the two hard modules kill them.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import sample_smooth_bodies_reference as SBR
from tests import smooth_bodies_jvp_reference as BJR
from tests import smooth_bodies_reference as BR
from tests.test_index_ranges_gpu import LAUNCH, around_the_cut
from tests.test_parity_gpu import assert_close, grid_to_dev, tol
from tests.test_smooth_hard_gpu import TILE, frozen, r32, tile_count, to

gpu = pytest.mark.gpu

DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 2)]
SHAPE = dict(B=65_600, P=300, grid=(8, 8), K=3)
GROUP_WORK = 2 ** 24  # kSmoothCloudsGroupWork of csrc/dpr_smooth.h


def group_rule(grid, P, B):
    """smooth_clouds_group with max_pose_group 0: min(B, 2^24 / max(P, tiles)) images are binned at once"""
    tiles = int(np.prod(tile_count(grid)))
    return max(1, min(B, GROUP_WORK // max(P, tiles)))


FIRST_GROUP = group_rule(SHAPE["grid"], SHAPE["P"], SHAPE["B"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(n_in, n_out):
    from tests.test_smooth_clouds_gpu import _poses
    B, P, grid, K = SHAPE["B"], SHAPE["P"], SHAPE["grid"], SHAPE["K"]
    rng = np.random.default_rng(7300 + 10 * n_in + n_out)
    rot, trans = _poses(rng, B * K, n_in, n_out)
    pts = rng.uniform(-1.0, 1.0, size=(P, n_in))
    pts[::25] *= 3.0  # some outside the grid
    c = SimpleNamespace(n_in=n_in, n_out=n_out, grid=grid, B=B, P=P, K=K, points=r32(pts),
                        body=rng.integers(0, K, P).astype(np.int64), rot=r32(rot.reshape(B, K, n_out, n_in)),
                        trans=r32(trans.reshape(B, K, n_out)), bg=r32(1.0 + np.arange(B) / B),
                        ow=r32(rng.uniform(0.5, 1.5, size=B)), pw=r32(rng.uniform(0.5, 1.5, size=P)))
    assert len(np.unique(c.bg.astype(np.float32))) == B
    assert min(len(np.unique(c.body[i:i + 64])) for i in range(0, 256, 64)) == K  # (every wave gathers its poses)
    frozen(c.points, c.body, c.rot, c.trans, c.bg, c.ow, c.pw)
    return c


def only_on(sel, a):
    """`a` (leading or trailing axis B) with zeros outside the images `sel`"""
    out = np.zeros_like(a)
    if a.shape[0] == SHAPE["B"]:
        out[sel] = a[sel]
    else:
        out[..., sel] = a[..., sel]
    return out


def rest_mask(sel, dev):
    rest = np.ones(SHAPE["B"], bool)
    rest[sel] = False
    return torch.as_tensor(rest, device=dev)


def primal(c, tdt, dev, ow):
    t = lambda a: to(a, tdt, dev)
    return [t(c.points), torch.as_tensor(np.array(c.body), device=dev), t(c.rot), t(c.trans), t(c.bg), t(ow), t(c.pw)]


def nan_buffers(c, tdt, dev, names):
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device=dev)
    bufs = dict(ds_dimage=dpr_amd.empty_grid(c.grid, c.B, tdt, dev).fill_(float("nan")), ds_dpoints=nan(c.P, c.n_in),
                ds_drotation=nan(c.B, c.K, c.n_in, c.n_out).transpose(-1, -2), ds_dtranslation=nan(c.B, c.K, c.n_out),
                ds_dbackground=nan(c.B), ds_dout_weight=nan(c.B), ds_dpoint_weight=nan(c.P))
    return {k: bufs[k] for k in names}


def check_pose_sums(got, want, sel, rest, npdt, what):
    """per (image, body) on the selected images; exactly 0 everywhere else"""
    assert bool(torch.isfinite(got).all()), f"non-finite {what}"
    for i, b in enumerate(sel):
        for k in range(want.shape[1]):
            assert float(np.abs(want[i, k]).max()) > 0
            assert_close(got[b, k], want[i, k].astype(npdt), tol(npdt, "pose"), f"{what}[{b}, {k}]")
    assert not bool((got[rest] != 0).any()), f"{what}: an image without sensitivity is not 0"


# ------------------------------------------------------------------ the CPU side
def test_the_shape_crosses_the_cuts_it_names():
    B, P, grid = SHAPE["B"], SHAPE["P"], SHAPE["grid"]
    assert B > LAUNCH + 1 and around_the_cut(B) == [0, 65534, 65535, 65536, 65599]
    # the image slices of the point kernels (note 1 of include/dpr.h, SUMMATION ORDER): 2 blocks, 1010 slices of 65
    blocks = -(-P // 256)
    per_slice = -(-B // min(B, -(-2048 // blocks), 65535))
    assert (blocks, per_slice, -(-B // per_slice), B - per_slice * (-(-B // per_slice) - 1)) == (2, 65, 1010, 15)
    # the group rule of the tiled forward
    assert int(np.prod(tile_count(grid))) == 1 and all(n <= e for n, e in zip(grid, TILE[2]))
    assert GROUP_WORK // P == 55_924 and FIRST_GROUP == min(B, 55_924) == 55_924 and B - FIRST_GROUP == 9_676
    assert FIRST_GROUP * blocks > LAUNCH  # (blocks of k_smooth_bodies_keys in one launch)
    assert set(tiled_images()) >= {FIRST_GROUP - 1, FIRST_GROUP, FIRST_GROUP + 1, LAUNCH - 1, LAUNCH, LAUNCH + 1}


def tiled_images():
    return sorted(set(around_the_cut(SHAPE["B"])) | {FIRST_GROUP - 1, FIRST_GROUP, FIRST_GROUP + 1})


# ------------------------------------------------------------------ the splat: forward, pullback, forward mode
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_smooth_bodies_images_across_the_launch_cuts(dev, npdt, tdt, n_in, n_out):
    c = case(n_in, n_out)
    sel = around_the_cut(c.B)
    rest = rest_mask(sel, dev)
    # forward: out_weight is non-zero only on the five images around the cut
    ow = only_on(sel, c.ow)
    args = primal(c, tdt, dev, ow)
    out = dpr_amd.raster_smooth_bodies(c.grid, *args, algo="atomic")
    assert tuple(out.shape) == c.grid + (c.B,) and out.dtype == tdt
    ref = BR.raster(c.grid, c.points, c.body, c.rot[sel], c.trans[sel], c.bg[sel], ow[sel], c.pw)
    for i, b in enumerate(sel):
        assert float(np.abs(ref[..., i] - c.bg[b]).max()) > 0.1
        assert_close(out[..., b], ref[..., i].astype(npdt), tol(npdt, "out"), f"out[.., {b}]")
    assert bool(((out == args[4]) | ~rest).all()), "an image of out_weight 0 is not its background"
    # pullback: ds_dout is non-zero only in those images; every out_weight is
    rng = np.random.default_rng(7400 + n_in)
    g = only_on(sel, r32(rng.normal(size=c.grid + (c.B,))))
    bufs = nan_buffers(c, tdt, dev, ("ds_dpoints", "ds_drotation", "ds_dtranslation", "ds_dbackground",
                                     "ds_dout_weight", "ds_dpoint_weight"))
    pb = dpr_amd.raster_pullback_smooth_bodies_(grid_to_dev(g.astype(npdt), dev), *primal(c, tdt, dev, c.ow), **bufs)
    want = BR.raster_pullback(g[..., sel], c.points, c.body, c.rot[sel], c.trans[sel], c.ow[sel], c.pw)
    assert pb.points.data_ptr() == bufs["ds_dpoints"].data_ptr()
    assert bool(torch.isfinite(pb.points).all()) and bool(torch.isfinite(pb.point_weight).all())
    assert_close(pb.points, want[0].astype(npdt), tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight, want[5].astype(npdt), tol(npdt, "points"), "ds_dpoint_weight")
    check_pose_sums(pb.rotation, want[1], sel, rest, npdt, "ds_drotation")
    check_pose_sums(pb.translation, want[2], sel, rest, npdt, "ds_dtranslation")
    check_pose_sums(pb.out_weight[:, None], want[4][:, None], sel, rest, npdt, "ds_dout_weight")
    check_pose_sums(pb.background[:, None], want[3][:, None], sel, rest, npdt, "ds_dbackground")


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_smooth_bodies_jvp_images_across_the_launch_cuts(dev, npdt, tdt, n_in, n_out):
    """V = 1, all six tangents; out_weight and out_weight_dot are non-zero only on the five images, so every other
    plane is background_dot[0, b] exactly."""
    c = case(n_in, n_out)
    sel = around_the_cut(c.B)
    rest = rest_mask(sel, dev)
    rng = np.random.default_rng(7500 + n_in)
    ow = only_on(sel, c.ow)
    t = dict(points_dot=rng.normal(size=(1, c.P, n_in)), rotation_dot=rng.normal(size=(1, c.B, c.K, n_out, n_in)),
             translation_dot=rng.normal(size=(1, c.B, c.K, n_out)), background_dot=(2.0 + np.arange(c.B) / c.B)[None],
             out_weight_dot=only_on(sel, rng.normal(size=c.B))[None], point_weight_dot=rng.normal(size=(1, c.P)))
    t = {k: r32(v) for k, v in t.items()}
    pts, body, rot, trans, _bg, dow, pw = primal(c, tdt, dev, ow)
    tan = {k: to(v, tdt, dev) for k, v in t.items()}
    out = dpr_amd.raster_smooth_bodies_jvp(c.grid, pts, body, rot, trans, None, dow, pw, tangents=1, algo="atomic",
                                           **tan)
    assert tuple(out.shape) == c.grid + (1, c.B) and out.dtype == tdt
    cut = lambda k, v: v if k in ("points_dot", "point_weight_dot") else v[:, sel]
    ref = BJR.raster_smooth_bodies_jvp(c.grid, c.points, c.body, c.rot[sel], c.trans[sel], ow[sel], c.pw, V=1,
                                       **{k: cut(k, v) for k, v in t.items()})
    for i, b in enumerate(sel):
        assert float(np.abs(ref[..., 0, i] - t["background_dot"][0, b]).max()) > 0.1
        assert_close(out[..., 0, b], ref[..., 0, i].astype(npdt), 1e-10 if npdt == np.float64 else 1e-4,
                     f"out_dot[.., 0, {b}]")
    assert bool(((out[..., 0, :] == tan["background_dot"][0]) | ~rest).all()), \
        "a plane without a tangent is not its background tangent"


@gpu
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tiled_forward_groups_across_the_launch_cuts(dev, n_in, n_out):
    """fp32, the default group rule: 55 924 images in the first group (111 848 blocks of k_smooth_bodies_keys, 55 924
    of k_smooth_bodies_tile), 9 676 in the second, from b0 = 55 924."""
    c = case(n_in, n_out)
    sel = tiled_images()
    rest = rest_mask(sel, dev)
    ow = only_on(sel, c.ow)
    args = primal(c, torch.float32, dev, ow)
    out = dpr_amd.raster_smooth_bodies(c.grid, *args, algo="tiled")
    ref = BR.raster(c.grid, c.points, c.body, c.rot[sel], c.trans[sel], c.bg[sel], ow[sel], c.pw)
    for i, b in enumerate(sel):
        assert float(np.abs(ref[..., i] - c.bg[b]).max()) > 0.1
        assert_close(out[..., b], ref[..., i].astype(np.float32), tol(np.float32, "out"), f"out[.., {b}]")
    assert bool(((out == args[4]) | ~rest).all()), "an image of out_weight 0 is not its background"


# ------------------------------------------------------------------ sampling: forward and atomic pullback
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_sample_smooth_bodies_images_across_the_launch_cuts(dev, npdt, tdt, n_in, n_out):
    c = case(n_in, n_out)
    sel = around_the_cut(c.B)
    rest = rest_mask(sel, dev)
    rng = np.random.default_rng(7600 + n_in)
    image = only_on(sel, r32(rng.normal(size=c.grid + (c.B,))))
    dv = only_on(sel, r32(rng.normal(size=(c.B, c.P)))).T  # (P, B)
    pts, body, rot, trans = primal(c, tdt, dev, c.ow)[:4]
    img = grid_to_dev(image.astype(npdt), dev)
    v = dpr_amd.sample_smooth_bodies(img, pts, body, rot, trans)
    assert tuple(v.shape) == (c.P, c.B) and v.dtype == tdt and v.t().is_contiguous()
    ref = SBR.sample(image[..., sel], c.points, c.body, c.rot[sel], c.trans[sel])
    for i, b in enumerate(sel):
        assert float(np.abs(ref[:, i]).max()) > 0.1
        assert_close(v[:, b], ref[:, i].astype(npdt), tol(npdt, "points"), f"values[:, {b}]")
    assert not bool((v.t()[rest] != 0).any()), "the column of a zero image is not 0"
    bufs = nan_buffers(c, tdt, dev, ("ds_dimage", "ds_dpoints", "ds_drotation", "ds_dtranslation"))
    pb = dpr_amd.sample_smooth_bodies_pullback_(to(dv.T, tdt, dev).t(), img, pts, body, rot, trans, algo="atomic",
                                                **bufs)
    assert pb.image.data_ptr() == bufs["ds_dimage"].data_ptr() and pb.points.data_ptr() == bufs["ds_dpoints"].data_ptr()
    want = SBR.sample_pullback(dv[:, sel], image[..., sel], c.points, c.body, c.rot[sel], c.trans[sel])
    assert bool(torch.isfinite(pb.points).all()) and bool(torch.isfinite(pb.image).all())
    assert_close(pb.points, want[1].astype(npdt), tol(npdt, "points"), "ds_dpoints")
    for i, b in enumerate(sel):
        assert float(np.abs(want[0][..., i]).max()) > 0
        assert_close(pb.image[..., b], want[0][..., i].astype(npdt), tol(npdt, "out"), f"ds_dimage[.., {b}]")
    assert bool(((pb.image == 0) | ~rest).all()), "ds_dimage: an image without sensitivity is not 0"
    check_pose_sums(pb.rotation, want[2], sel, rest, npdt, "ds_drotation")
    check_pose_sums(pb.translation, want[3], sel, rest, npdt, "ds_dtranslation")
