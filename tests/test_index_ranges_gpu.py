"""Launch-size cuts and offsets past 2^32 in the op families (channels, JVP, sampling, per-pose clouds, ORDERED, the
smooth splat, smooth sampling).

Part A: plane / pose counts across the cuts at 65535 (grid.y), 2^20 (k_ord_reduce blocks) and 256 (the LDS staging
round of k_ord_reduce), on tiny grids.  Part B: a whole plane, pose or cloud past element 2^32 (fp32, 17 GB arrays:
the smallest size at which a 32-bit offset can show).  Each test asserts on its own shape that it crosses the limit it
names; test_shapes_cross_the_limit_they_name_and_no_other recomputes that on the CPU from include/dpr.h.

What guards what (csrc/dpr_api.hip, or the family's own csrc/dpr_api_*.hip, unless another file is named):

  fill_background    `out + k0 * G`, `bg + k0`, cut inside a pose    test_channels_planes_across_the_launch_cut
                     cut between poses                               test_channels_poses_across_the_pose_stride,
                                                                     test_clouds_poses_across_the_launch_cuts,
                                                                     test_smooth_poses_across_the_launch_cuts
  grid_sum           `g + k0 * G`, `d_bg + k0`                       test_channels_planes_across_the_launch_cut,
                                                                     test_clouds_poses_across_the_launch_cuts,
                                                                     test_smooth_poses_across_the_launch_cuts
  k_fwd_atomic_ch    pose stride over gridDim.y = 65535              test_channels_poses_across_the_pose_stride
  jvp_fill           `q0` loop; k_jvp_fill: q -> bg_dot[k * B + b]   test_jvp_planes_across_the_launch_cut
  k_clouds_fwd_atomic, k_clouds_bwd_atomic: pose stride              test_clouds_poses_across_the_launch_cuts
  k_clouds_fwd_tile, k_clouds_bwd_tile, k_clouds_reduce: `b0`        test_clouds_poses_across_the_launch_cuts
  pullback_ordered   (dpr_ordered.hip) `g + b0 * G`, `rk.target += b0 * G`, `part_grid + b0 * gchunks * 2`, and
                     k_ord_reduce's stride over 2^20 blocks:
                                            test_ordered_poses_across_the_launch_cut_and_the_reduce_stride
  k_ord_reduce       second staging round, point chunks              test_ordered_reduce_second_round_of_point_chunks
                     second staging round, cell chunks (and loss)    test_ordered_reduce_second_round_of_cell_chunks
  k_smooth_fwd_atomic (dpr_smooth.hip) pose stride over gridDim.y    test_smooth_poses_across_the_launch_cuts
  k_smooth_bwd       (dpr_smooth.hip) `b_lo = blockIdx.y * poses_per_slice`, 1010 slices of 65 poses
                                                                     test_smooth_poses_across_the_launch_cuts
  (b * C + c) * G    channels TILED and ATOMIC, (3, 3)               test_channels_planes_past_2_pow_32
  (b * K + k) * G    JVP TILED and ATOMIC, (3, 3)                    test_jvp_planes_past_2_pow_32
  b * G              image and ds_dimage, sampling ATOMIC / TILED    test_sample_image_past_2_pow_32
  b * P              values, sampling forward                        test_sample_values_past_2_pow_32
  b * G              clouds TILED, ATOMIC and CHUNKED                test_clouds_out_past_2_pow_32
  b * P * NI         clouds ATOMIC and CHUNKED                       test_clouds_points_past_2_pow_32
  b * G              ORDERED forward and pullback                    test_ordered_pose_past_2_pow_32
  b * G              smooth ATOMIC and TILED forward (k_smooth_fwd_atomic, k_smooth_tile), ATOMIC pullback
                     (k_smooth_bwd), (3, 3)                          test_smooth_pose_past_2_pow_32
  k_sample_smooth_fwd, k_sample_smooth_bwd (dpr_smooth.hip) `b_lo = blockIdx.y * poses_per_slice`, 1010 slices of 65
                     poses, the last of 15 (the b_hi clamp), B > 65535
                                                                     test_sample_smooth_poses_across_the_launch_cuts
  b * G              image (k_sample_smooth_fwd, k_sample_smooth_bwd), ds_dimage (k_sample_smooth_bwd; the driver's
                     `d_img + b * G` for the TILED planes), (3, 3)   test_sample_smooth_image_past_2_pow_32
  b * P              values (k_sample_smooth_fwd), ds_dvalues (k_sample_smooth_bwd; the driver's `dv + b * P` for the
                     TILED planes), (3, 3)                           test_sample_smooth_values_past_2_pow_32

Not reachable: the JVP's tangent offset k * P * NI stays below 2^32 at the 16-tangent limit even for P = 2^23,
NI = 3 (15 * 2^23 * 3 = 1.4 * 2^28), so that second, small-grid call is left out; the (K, P, NI) tangents of
test_jvp_planes_past_2_pow_32 are read at their small offsets only.

Part A selects planes / poses 0, 65534, 65535, 65536 and the last, and adds one device-side check of the whole
tensor.  test_ordered_poses_across_the_launch_cut_and_the_reduce_stride gives only the five selected poses a
sensitivity in its plain pullback (the serial oracle needs 6.6 s for all 70 000 poses); its residual pullback runs
on a dense batch.  The ten *_past_2_pow_32 tests sit at the 2^32 floor: 17 GB arrays are their point.
The smooth splat's TILED forward is left out of Part A: it launches four kernels per pose from the host (262 400
launches at B = 65 600) and its per-pose loop has no cut; its `b * G` is in Part B.  The TILED smooth sampling
pullback is left out of Part A for the same reason (its planes are that forward, pose by pose); its `d_img + b * G`
and `dv + b * P` are in Part B.  test_sample_smooth_values_past_2_pow_32 gives ds_dvalues[:, 256] a value at 100 000
of its 2^24 points only: the numpy reference walks the 27 cells of every point with a sensitivity, far beyond a
test's seconds for all of them, and a wrapped offset reads the zeros of an earlier column at those points as well.
Wall time on an MI355X (2026-10-19): test_sample_smooth_image_past_2_pow_32 1.5 s (test_sample_image_past_2_pow_32
0.7 s, test_smooth_pose_past_2_pow_32 0.9 s); test_sample_smooth_values_past_2_pow_32 2.4 s
(test_sample_values_past_2_pow_32, forward only, 0.1 s after it and 1.0 s when it runs first).

Mutation record (scratch builds of libdpr, one MI355X run each; every mutant keeps its accesses inside the buffers,
a truncated offset wraps DOWN).  Each line: the mutant, the test it failed, the first assertion that fired.
  fill_background `bg + k0` -> `bg`            channels_planes: plane 65535 = (pose 4095, channel 15); channels_poses:
                                               pose 65534; clouds_poses: out[.., 65535]
  k_jvp_fill bg_dot[k * B + b] -> [b * K + k]  jvp_planes (all four): a plane (b, k) is not background_dot[k, b]
  pullback_ordered without `rk.target += ..`   ordered_poses: residual, pose 65535 alone: background (plain part passes)
  k_ord_reduce, first staging round only       second_round_of_point_chunks: rotation off by 4.5e-3 (dense case);
                                               second_round_of_cell_chunks: background off by 9.6e-2
  k_fwd_atomic_ch `b += gridDim.y` -> no stride   channels_poses: pose 65535, channel 0
  grid_sum `g + k0 * G` -> `g`                 channels_planes: ds_dbackground, 65 of 65600 plane sums, first (0, 4096)
  k_clouds_reduce without `b0`                 clouds_poses: ds_drotation[65535] (100 % off)
  32-bit (b * C) * G in k_fwd_atomic_ch        channels_planes_past: atomic, pose 16 channel 0 (TILED passes before)
  32-bit b * K * G in k_jvp_atomic             jvp_planes_past: atomic, pose 16 tangent 0
  32-bit b * G (image), b * P in k_sample_fwd  sample_image_past: values[:, 256]; sample_values_past:
                                               values[subsample, 256]
  32-bit b * P * NI, b * G, k_clouds_fwd_atomic   clouds_points_past: atomic out[.., 342]; clouds_out_past: atomic
                                               out[.., 256]
  32-bit b * G in k_ord_gather                 ordered_pose_past: out[.., 256], all 16 777 216 cells differ
  k_clouds_fwd_tile without `b0`               clouds_poses: chunked out[.., 65535] (atomic passes before)
  k_ord_reduce without its stride              ordered_poses: pose 69999 alone: rotation, the batch's row never written
  32-bit b * C * G (ds_dout), k_bwd_gather_ch  channels_planes_past: ds_dpoint_weight[:, 0] (100 % off)
  32-bit b * G (ds_dimage) in k_sample_bwd     sample_image_past: atomic ds_dimage[.., 256]
  32-bit b * G (ds_dout), k_clouds_bwd_atomic  clouds_out_past: atomic ds_dpoints[256]
  32-bit b * G (out) in k_clouds_fwd_tile      clouds_out_past: chunked out[.., 256] (100 % off)
  32-bit b * G (ds_dout) in k_clouds_bwd_tile  clouds_out_past: chunked ds_dpoints[256]
  32-bit b * P * NI in k_clouds_bwd_atomic     clouds_points_past: atomic ds_dpoints[342]
  32-bit b * G (ds_dout) in k_ord_bwd          ordered_pose_past: ds_dpoints, 286 389 of 300 000 elements differ
  k_smooth_fwd_atomic `b += gridDim.y` -> no stride   smooth_poses: out[.., 65535] (77 % off; poses 0 and 65534 pass before)
  32-bit b * G (out) in k_smooth_fwd_atomic    smooth_pose_past: atomic: out[.., 256]
  32-bit b * G (out) in k_smooth_tile          smooth_pose_past: tiled: out[.., 256] (ATOMIC passes before)
  32-bit b * G (ds_dout) in k_smooth_bwd       smooth_pose_past: ds_dpoints (100 % off; both forwards pass before)
(The smooth sampling mutants: tests/test_sample_smooth_hard_gpu.py.)
Argued from the code, not run: the `out + k0 * G` / `d_bg + k0` halves of the two driver cuts, k_clouds_bwd_tile's
`b0` and the strides of k_clouds_fwd_atomic / k_clouds_bwd_atomic (the idioms above, in kernels whose wrong pose
would show in the same assertions), and every mutant that moves an access past its allocation."""
import os
import re

import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests import sample_smooth_reference as SSR
from tests import smooth_reference as SR
from tests.test_channels_gpu import tol as channels_tol
from tests.test_clouds_gpu import check_against_oracle as clouds_check_against_oracle
from tests.test_clouds_gpu import tol as clouds_tol
from tests.test_jvp_abi import jvp_reference, random_tangents
from tests.test_jvp_gpu import tol as jvp_tol
from tests.test_ordered_gpu import POSE_FIELDS, assert_same_bits, grid_to_dev, pose_args, pullback_ordered
from tests.test_ordered_gpu import tol as ordered_tol
from tests.test_parity_gpu import tol as smooth_tol
from tests.test_sample_gpu import tol as sample_tol

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "dpr.h")).read()
POINT_CHUNK = int(re.search(r"#define DPR_ORDERED_POINT_CHUNK (\d+)", _HEADER).group(1))
CELL_CHUNK = int(re.search(r"#define DPR_ORDERED_CELL_CHUNK (\d+)", _HEADER).group(1))
LAUNCH = 65535  # poses or planes on grid.y of one launch
REDUCE_BLOCKS = 2 ** 20  # blocks of k_ord_reduce, which then stride
STAGE = 256  # chunk partials k_ord_reduce stages through LDS per round
DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
F32 = np.float32

# every shape of this module (the CPU test walks them)
A_CHANNELS_PLANES = dict(C=16, B=4100, grid=(8, 8), P=300, n_in=3)
A_CHANNELS_POSES = dict(C=2, B=65_600, grid=(8, 8), P=300, n_in=3)
A_JVP_PLANES = dict(K=16, B=4100, grid=(8, 8), P=300)
A_JVP_POSES = dict(K=1, B=65_600, grid=(8, 8), P=300)
A_CLOUDS = dict(B=65_600, P=16, grid=(16, 16))
A_ORDERED = dict(B=70_000, P=300, grid=(4, 4, 4), n_in=3)
A_ORD_POINTS = dict(B=2, P=257 * POINT_CHUNK + 17, grid=(8, 8, 8), n_in=3)
A_ORD_CELLS = dict(B=2, P=3000, grid=(162, 162, 162), n_in=3)
A_SMOOTH = dict(B=65_600, P=300, grid=(8, 8))
B_CHANNELS = dict(C=16, B=17, grid=(256,) * 3, P=100_000)
B_JVP = dict(K=16, B=17, grid=(256,) * 3, P=100_000)
B_SAMPLE_IMAGE = dict(B=257, grid=(256,) * 3, P=100_000)
B_SAMPLE_VALUES = dict(B=257, grid=(16,) * 3, P=2 ** 24)
B_CLOUDS_OUT = dict(B=257, grid=(256,) * 3, P=20_000)
B_CLOUDS_POINTS = dict(B=343, grid=(16, 16), P=2 ** 22, n_in=3)
B_ORDERED = dict(B=257, grid=(256,) * 3, P=100_000)
B_SMOOTH = dict(B=257, grid=(256,) * 3, P=100_000)
A_SAMPLE_SMOOTH = dict(B=65_600, P=300, grid=(8, 8))
B_SAMPLE_SMOOTH_IMAGE = dict(B=257, grid=(256,) * 3, P=100_000)
B_SAMPLE_SMOOTH_VALUES = dict(B=257, grid=(16,) * 3, P=2 ** 24)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def cells(grid):
    return int(np.prod(grid))


def around_the_cut(n):
    """Indices on both sides of a cut at 65535, the first and the last."""
    assert n > LAUNCH + 1
    return [0, LAUNCH - 1, LAUNCH, LAUNCH + 1, n - 1]


def assert_close(actual, expected, rtol, what=""):
    if isinstance(actual, torch.Tensor) and actual.is_cuda and actual.numel() >= 2 ** 20:
        return assert_close_on_device(actual, expected, rtol, what)
    a = actual.detach().cpu().numpy() if isinstance(actual, torch.Tensor) else np.asarray(actual)
    e = expected.detach().cpu().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    a, e = a.astype(np.float64), e.astype(np.float64)
    assert np.all(np.isfinite(a)), f"{what}: non-finite values"
    err = np.linalg.norm((a - e).ravel())
    scale = max(np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel()))
    assert err <= rtol * scale + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


def assert_close_on_device(actual, expected, rtol, what):
    """assert_close for a whole 256^3 plane: the norms are formed on the device in fp64"""
    e = expected if isinstance(expected, torch.Tensor) else torch.as_tensor(expected)
    assert tuple(actual.shape) == tuple(e.shape), f"{what}: shape {tuple(actual.shape)} != {tuple(e.shape)}"
    a, e = actual.detach().double(), e.to(actual.device).double()
    assert bool(torch.isfinite(a).all()), f"{what}: non-finite values"
    err, scale = float((a - e).norm()), max(float(a.norm()), float(e.norm()))
    assert err <= rtol * scale + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


def assert_plane_sums(got, g, n_out, npdt, what):
    """got[k] against the sum of plane k of `g` (grid axes first), formed on the device in fp64, for EVERY plane.
    Bound per plane: a sum of G terms in the working type, in any order, errs by at most G eps sum |x|."""
    dims = tuple(range(n_out))
    gd = g.double()
    want, mag = gd.sum(dims), gd.abs().sum(dims)
    G = cells(g.shape[:n_out])
    bound = (G * float(np.finfo(npdt).eps)) * mag + 1e-300
    err = (got.double() - want).abs()
    assert err.shape == bound.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} plane sums are off; first at " \
        f"{tuple(int(v) for v in bad.nonzero()[0])}"


def max_plane_error(a, b, n_out):
    """max over planes of |a - b| / max(|a|, |b|) (2-norms over the grid axes), on the device."""
    dims = tuple(range(n_out))
    ad, bd = a.double(), b.double()
    err = (ad - bd).pow(2).sum(dims).sqrt()
    scale = torch.maximum(ad.pow(2).sum(dims).sqrt(), bd.pow(2).sum(dims).sqrt()).clamp_min(1e-300)
    return float((err / scale).max())


def distinct(n, lo_bits):
    """n distinct values centred on 0, exact in fp32: multiples of 2^-lo_bits."""
    assert n < 2 ** 23
    return (np.arange(n, dtype=np.float64) - n // 2) / 2.0 ** lo_bits


# =================================================================== Part A
# ------------------------------------------------------------------ A.1 channels: B * C planes
def channels_case(npdt, shape, seed):
    C, B, grid, P = shape["C"], shape["B"], shape["grid"], shape["P"]
    d = D.make(n_points=P, n_in=shape["n_in"], n_out=len(grid), batch=B, grid_n=grid, seed=seed, dtype=npdt)
    rng = np.random.default_rng(seed + 100)
    d.pw = np.asarray(rng.uniform(0.2, 1.0, size=(P, C)) * (1.0 + np.arange(C)), dtype=npdt)
    d.bg = np.asarray(distinct(B * C, 14).reshape(B, C), dtype=npdt)  # bg[b, c]: plane b * C + c, within +-4.1
    assert len(np.unique(d.bg)) == B * C
    return d


def oracle_channel_plane(oracle, d, b, c, npdt):
    return oracle.raster(d.grid, d.points, d.rotations[b:b + 1], d.translations[b:b + 1], d.bg[b, c:c + 1],
                         d.weights[b:b + 1], d.pw[:, c], dtype=npdt)[..., 0]


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_channels_planes_across_the_launch_cut(oracle, dev, npdt, tdt):
    s = A_CHANNELS_PLANES
    C, B, grid, P = s["C"], s["B"], s["grid"], s["P"]
    planes = B * C
    assert planes > LAUNCH and B <= LAUNCH  # the plane cut, not the pose stride
    assert LAUNCH % C != 0  # the cut falls inside a pose: plane 65535 is pose 4095, channel 15
    d = channels_case(npdt, s, seed=1)
    pts, R, t, pw, bg, ow = (T(a, dev) for a in (d.points, d.rotations, d.translations, d.pw, d.bg, d.weights))
    out = dpr_amd.raster_channels(grid, pts, R, t, pw, bg, ow, algo="atomic")
    assert tuple(out.shape) == grid + (C, B) and out.dtype == tdt
    for k in around_the_cut(planes):
        b, c = divmod(k, C)
        assert_close(out[..., c, b], oracle_channel_plane(oracle, d, b, c, npdt), channels_tol(npdt, "out"),
                     f"plane {k} = (pose {b}, channel {c})")
    # whole tensor: without points every plane is its background, exactly
    empty = dpr_amd.raster_channels(grid, pts[:0], R, t, pw[:0], bg, ow, algo="atomic")
    assert torch.equal(empty, bg.t().expand(grid + (C, B))), "P = 0: a plane is not its background"
    # pullback
    gen = torch.Generator(device=dev).manual_seed(2)
    g = torch.randn((B, C) + grid[::-1], generator=gen, dtype=tdt, device=dev).permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_channels_(g, pts, R, t, pw, bg, ow, algo="atomic")
    torch.cuda.synchronize()
    assert_plane_sums(pb.background.t(), g, 2, npdt, "ds_dbackground")
    gn = g.cpu().numpy()
    sums = None
    for c in range(C):  # the oracle composed per channel, over all poses
        r = oracle.raster_pullback(gn[..., c, :], d.points, d.rotations, d.translations, d.weights, d.pw[:, c],
                                   dtype=npdt)
        assert_close(pb.point_weight[:, c], r.point_weight, channels_tol(npdt, "points"), f"ds_dpoint_weight[:, {c}]")
        parts = [np.asarray(x, np.float64) for x in (r.points, r.rotation, r.translation, r.out_weight)]
        sums = parts if sums is None else [a + x for a, x in zip(sums, parts)]
    assert_close(pb.points, sums[0], channels_tol(npdt, "points"), "ds_dpoints")
    poses = sorted({k // C for k in around_the_cut(planes)})
    for name, got, want in (("ds_drotation", pb.rotation, sums[1]), ("ds_dtranslation", pb.translation, sums[2]),
                            ("ds_dout_weight", pb.out_weight, sums[3])):
        assert_close(got, want, channels_tol(npdt, "pose"), name)
        for b in poses:
            assert_close(got[b:b + 1], want[b:b + 1], channels_tol(npdt, "pose"), f"{name}[{b}]")


# ------------------------------------------------------------------ A.2 channels: B poses
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_channels_poses_across_the_pose_stride(oracle, dev, npdt, tdt):
    s = A_CHANNELS_POSES
    C, B, grid = s["C"], s["B"], s["grid"]
    assert B > LAUNCH  # k_fwd_atomic_ch strides over gridDim.y = 65535 poses
    d = channels_case(npdt, s, seed=3)
    pts, R, t, pw, bg, ow = (T(a, dev) for a in (d.points, d.rotations, d.translations, d.pw, d.bg, d.weights))
    out = dpr_amd.raster_channels(grid, pts, R, t, pw, bg, ow, algo="atomic")
    for b in around_the_cut(B):
        for c in range(C):
            assert_close(out[..., c, b], oracle_channel_plane(oracle, d, b, c, npdt), channels_tol(npdt, "out"),
                         f"pose {b}, channel {c}")
    empty = dpr_amd.raster_channels(grid, pts[:0], R, t, pw[:0], bg, ow, algo="atomic")
    assert torch.equal(empty, bg.t().expand(grid + (C, B))), "P = 0: a plane is not its background"
    # whole tensor: every plane against the single-channel direct kernel, plane by plane
    for c in range(C):
        ref = dpr_amd.raster(grid, pts, R, t, bg[:, c].contiguous(), ow, pw[:, c].contiguous(), algo="atomic")
        worst = max_plane_error(out[..., c, :], ref, 2)
        assert worst <= channels_tol(npdt, "out"), f"channel {c}: worst plane off by {worst:.3e}"


# ------------------------------------------------------------------ A.3 JVP: B * K planes
class JvpCase:
    def __init__(self, dev, npdt, tdt, n_in, n_out, shape, seed):
        K, B, grid, P = shape["K"], shape["B"], shape["grid"], shape["P"]
        d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=seed, dtype=npdt)
        rng = np.random.default_rng(seed + 17)
        r = lambda a: np.asarray(a, dtype=npdt).astype(np.float64)
        self.grid, self.K, self.B, self.npdt = grid, K, B, npdt
        self.points, self.rot, self.trans = r(d.points), r(d.rotations), r(d.translations)
        self.ow, self.pw = r(rng.uniform(0.5, 2.0, size=B)), r(rng.uniform(0.5, 2.0, size=P))
        self.tan = {k: r(v) for k, v in random_tangents(rng, K, P, B, n_in, n_out).items()}
        self.tan["background"] = r(distinct(K * B, 8).reshape(K, B))  # bg_dot[k, b]: distinct, exact
        to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
        self.primal = tuple(to(a) for a in (self.points, self.rot, self.trans)) + (None, to(self.ow), to(self.pw))
        self.kw = {k + "_dot": to(v) for k, v in self.tan.items()}

    def reference(self, poses):
        """(grid..., K, len(poses)): the restatement for the selected poses"""
        per_pose = ("rotation", "translation", "background", "out_weight")
        tan = {k: (v[:, poses] if k in per_pose else v) for k, v in self.tan.items()}
        return jvp_reference(self.grid, self.points, self.rot[poses], self.trans[poses], self.ow[poses], self.pw, tan,
                             self.K, cell_dtype=self.npdt)


def check_jvp_case(c, planes):
    K, B = c.K, c.B
    # only the background tangent: plane (b, k) is bg_dot[k, b] -- the transposed index -- over the whole tensor
    only = dpr_amd.raster_jvp(c.grid, *c.primal, background_dot=c.kw["background_dot"], tangents=K, algo="atomic")
    assert tuple(only.shape) == tuple(c.grid) + (K, B)
    assert torch.equal(only, c.kw["background_dot"].expand(tuple(c.grid) + (K, B))), \
        "a plane (b, k) is not background_dot[k, b]"
    out = dpr_amd.raster_jvp(c.grid, *c.primal, **c.kw, tangents=K, algo="atomic")
    poses = sorted({q // K for q in planes})
    ref = c.reference(poses)
    got = out[..., T(np.asarray(poses), out.device)]
    for i, b in enumerate(poses):
        for k in range(K):
            assert_close(got[..., k, i], ref[..., k, i], jvp_tol(c.npdt),
                         f"plane {b * K + k} = (pose {b}, tangent {k})")


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(3, 2), (2, 2)])
def test_jvp_planes_across_the_launch_cut(dev, npdt, tdt, n_in, n_out):
    s = A_JVP_PLANES
    assert s["B"] * s["K"] > LAUNCH and s["B"] <= LAUNCH and LAUNCH % s["K"] != 0
    check_jvp_case(JvpCase(dev, npdt, tdt, n_in, n_out, s, seed=5), around_the_cut(s["B"] * s["K"]))
    s = A_JVP_POSES
    assert s["B"] > LAUNCH and s["K"] == 1
    check_jvp_case(JvpCase(dev, npdt, tdt, n_in, n_out, s, seed=6), around_the_cut(s["B"]))


# ------------------------------------------------------------------ A.4 per-pose clouds: B poses
def cloud_batch(n_in, n_out, shape, seed):
    """The dict of tests/test_clouds_gpu.py::clouds, built without a loop over the poses: a different cloud, spread,
    background and weight per pose; a few points outside the grid."""
    B, P, grid = shape["B"], shape["P"], tuple(shape["grid"])
    rng = np.random.default_rng(seed)
    d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=seed)
    pts = (0.15 + 0.4 * rng.uniform(size=(B, 1, 1))) * rng.normal(size=(B, P, n_in))
    pts[:, 0] *= 6.0
    bg = distinct(B, 14)
    assert len(np.unique(bg.astype(np.float32))) == B
    return dict(grid=grid, points=pts, rot=d.rotations, trans=d.translations, pw=rng.uniform(0.5, 1.5, size=(B, P)),
                bg=bg, ow=rng.uniform(1, 10, size=B), ds=np.asarray(d.ds_dout), B=B, P=P)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(3, 2), (2, 2)])
def test_clouds_poses_across_the_launch_cuts(oracle, dev, npdt, tdt, n_in, n_out):
    s = A_CLOUDS
    B = s["B"]
    assert B > LAUNCH
    c = cloud_batch(n_in, n_out, s, seed=10 * n_in + n_out)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    t = {k: to(c[k]) for k in ("points", "rot", "trans", "pw", "bg", "ow")}
    ds = dpr_amd.to_grid_layout(to(c["ds"]))
    res = {}
    for algo in ("atomic", "chunked"):
        out = dpr_amd.raster_clouds(c["grid"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"], algo=algo)
        pb = dpr_amd.raster_pullback_clouds_(ds, t["points"], t["rot"], t["trans"], t["bg"], t["ow"], t["pw"],
                                             algo=algo)
        torch.cuda.synchronize()
        clouds_check_against_oracle(c, out, pb, npdt, poses=around_the_cut(B))
        assert_plane_sums(pb.background, ds, n_out, npdt, f"{algo}: ds_dbackground")
        res[algo] = (out, pb)
    # whole batch: the pose-owned tiles against the direct kernels
    (oa, pa), (oc, pc) = res["atomic"], res["chunked"]
    worst = max_plane_error(oc, oa, n_out)
    assert worst <= clouds_tol(npdt, "out"), f"out: worst plane off by {worst:.3e}"
    for name, kind in (("points", "points"), ("point_weight", "points"), ("rotation", "pose"),
                       ("translation", "pose"), ("out_weight", "pose")):
        assert_close(getattr(pc, name), getattr(pa, name), clouds_tol(npdt, kind), f"chunked vs atomic: {name}")
    # ... and pose by pose, so that no single pose hides in the norm of 65 600: the vector-valued gradients of a pose
    # against another pose's (or zeros) differ by about their own norm; a sum of 16 points' terms in the working type
    # cannot come near half of it.  (The scalar ds_dout_weight too: 64 terms of one pose cancel to 1e-2 of their
    # magnitude at the worst among 65 600 poses, far above the rounding of the sum.)
    for name in ("points", "point_weight", "rotation", "translation", "out_weight"):
        worst = max_plane_error(getattr(pc, name).reshape(B, -1).t(), getattr(pa, name).reshape(B, -1).t(), 1)
        assert worst <= 0.5, f"{name}: a pose of the chunked result is not the atomic one's ({worst:.3e})"


# ------------------------------------------------------------------ A.5 ORDERED pullback: B poses, 2^20 reduce items
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_ordered_poses_across_the_launch_cut_and_the_reduce_stride(oracle, dev, npdt, tdt):
    s = A_ORDERED
    B, P, grid = s["B"], s["P"], s["grid"]
    NV = 3 * 3 + 3 + 1
    assert NV == 13 and B > LAUNCH and B * (NV + 2) > REDUCE_BLOCKS
    d = D.make(n_points=P, n_in=3, n_out=3, batch=B, grid_n=grid, seed=50, dtype=npdt)
    sel = around_the_cut(B)
    # The serial oracle takes 6.6 s for 70 000 poses of 300 points, so the plain pullback runs on a batch in which
    # only the five selected poses have a sensitivity: the point gradients are then the oracle's over those five, in
    # index order (a pose without sensitivity adds +-0 to a running sum), and every other pose's sums are exactly 0.
    # The residual pullback below runs on a dense batch.
    rest = np.ones(B, dtype=bool)
    rest[sel] = False
    dense = d.ds_dout.copy(order="F")
    d.ds_dout[..., rest] = 0
    pb = pullback_ordered(d, dev)
    ref = oracle.raster_pullback(d.ds_dout[..., sel], d.points, d.rotations[sel], d.translations[sel], d.weights[sel],
                                 d.point_weights, dtype=npdt)
    assert_same_bits(pb.points, ref.points, "ds_dpoints")
    assert_same_bits(pb.point_weight, ref.point_weight, "ds_dpoint_weight")
    # a pose's sums depend neither on B nor on its position
    for b in sel:
        alone = pullback_ordered(d, dev, sel=[b])
        for name in POSE_FIELDS:
            assert_same_bits(getattr(alone, name)[0], getattr(pb, name)[b], f"pose {b} alone: {name}")
    # whole batch: the selected poses hold the oracle's values, every other pose exact zeros
    isel, irest = T(np.asarray(sel), dev), T(rest, dev)
    for name in POSE_FIELDS:
        assert_close(getattr(pb, name)[isel], getattr(ref, name), ordered_tol(npdt, "pose"), name)
        assert float(np.abs(getattr(ref, name)).min()) > 0
        assert not bool((getattr(pb, name)[irest] != 0).any()), f"{name}: a pose without sensitivity is not 0"
    d.ds_dout[...] = dense
    # the residual pullback: `target` is advanced per launch
    args = pose_args(d, dev)
    gen = torch.Generator(device=dev).manual_seed(51)
    out = torch.randn((B,) + grid[::-1], generator=gen, dtype=tdt, device=dev).permute(3, 2, 1, 0)
    target = grid_to_dev(d.ds_dout, dev)
    got, loss = dpr_amd.raster_residual_pullback_(out, target, *args, scale=0.7, algo="ordered")
    torch.cuda.synchronize()
    for b in sel:
        one = [a if a.shape[0] == P else a[b:b + 1] for a in args]
        g1, l1 = dpr_amd.raster_residual_pullback_(out[..., b:b + 1], target[..., b:b + 1], *one, scale=0.7,
                                                   algo="ordered")
        for name in POSE_FIELDS:
            assert_same_bits(getattr(g1, name)[0], getattr(got, name)[b], f"residual, pose {b} alone: {name}")
        assert_same_bits(l1[0], loss[b], f"residual, pose {b} alone: loss")
    resid = out - target
    assert_plane_sums(loss, resid * resid, 3, npdt, "loss")
    want = dpr_amd.raster_pullback_(dpr_amd.to_grid_layout(torch.tensor(0.7, dtype=tdt, device=dev) * resid), *args,
                                    algo="ordered")
    for name, a, e in zip(got._fields, got, want):
        assert_same_bits(a, e, f"residual against the pullback of its sensitivity: {name}")


# ------------------------------------------------------------------ A.6 k_ord_reduce: the second staging round
def check_ordered_batch(oracle, dev, d, npdt):
    """What k_ord_reduce writes (the per-pose sums, ds_dbackground) against the fp64 oracle; same bits for a pose
    alone, in the batch and with the batch reversed.  The point gradients, which do not pass through the reduction,
    are held to the contract instead: the bits of the serial oracle in the working type.  (Against the fp64 oracle
    the fp32 ds_dpoints of the 526 353-point cloud are 1.54e-3 off, the serial fp32 oracle's own figure: one point
    whose cell differs between fp32 and fp64 arithmetic, where the gradient jumps.  ds_dpoint_weight has no jump.)"""
    B = d.batch
    pb = pullback_ordered(d, dev)
    r64 = lambda a: np.asarray(a, np.float64)
    ref = oracle.raster_pullback(r64(d.ds_dout), r64(d.points), r64(d.rotations), r64(d.translations),
                                 r64(d.weights), r64(d.point_weights), dtype=np.float64)
    for name in POSE_FIELDS:
        assert_close(getattr(pb, name), getattr(ref, name), ordered_tol(npdt, "pose"), name)
    assert_close(pb.point_weight, ref.point_weight, ordered_tol(npdt, "points"), "ds_dpoint_weight")
    same = ref if npdt == np.float64 else oracle.raster_pullback(
        d.ds_dout, d.points, d.rotations, d.translations, d.weights, d.point_weights, dtype=npdt)
    assert_same_bits(pb.points, same.points, "ds_dpoints")
    assert_same_bits(pb.point_weight, same.point_weight, "ds_dpoint_weight")
    for b in range(B):
        alone = pullback_ordered(d, dev, sel=[b])
        for name in POSE_FIELDS:
            assert_same_bits(getattr(alone, name)[0], getattr(pb, name)[b], f"pose {b} alone: {name}")
    rev = pullback_ordered(d, dev, sel=list(range(B))[::-1])
    for name in POSE_FIELDS:
        assert_same_bits(getattr(rev, name).flip(0), getattr(pb, name), f"reversed batch: {name}")
    return pb, ref


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_ordered_reduce_second_round_of_point_chunks(oracle, dev, npdt, tdt):
    s = A_ORD_POINTS
    P = s["P"]
    pchunks = -(-P // POINT_CHUNK)
    assert STAGE < pchunks <= 2 * STAGE and P % POINT_CHUNK != 0
    d = D.make(n_points=P, n_in=3, n_out=3, batch=s["B"], grid_n=s["grid"], seed=60, dtype=npdt)
    check_ordered_batch(oracle, dev, d, npdt)
    # only the second round holds anything: the points of chunks 0 .. 255 lie outside every grid
    first = STAGE * POINT_CHUNK
    d.points[:first] = 9.0
    pb, ref = check_ordered_batch(oracle, dev, d, npdt)
    assert float(np.abs(ref.rotation).min()) > 0 and not bool((pb.points[:first] != 0).any())


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_ordered_reduce_second_round_of_cell_chunks(oracle, dev, npdt, tdt):
    s = A_ORD_CELLS
    B, grid = s["B"], s["grid"]
    G = cells(grid)
    gchunks = -(-G // CELL_CHUNK)
    assert STAGE < gchunks <= 2 * STAGE
    d = D.make(n_points=s["P"], n_in=3, n_out=3, batch=B, grid_n=grid, seed=61, dtype=npdt)
    check_ordered_batch(oracle, dev, d, npdt)
    # only the second round holds anything: ds_dout (and the residual) is zero outside the cell chunks >= 256
    flat = d.ds_dout.reshape(G, B, order="F")  # (a view: cell index in memory order)
    assert np.shares_memory(flat, d.ds_dout)
    flat[:STAGE * CELL_CHUNK] = 0
    assert not d.ds_dout.ravel(order="F").reshape(B, G)[:, :STAGE * CELL_CHUNK].any()
    assert float(np.abs(d.ds_dout).sum()) > 0
    pb, ref = check_ordered_batch(oracle, dev, d, npdt)
    assert float(np.abs(ref.background).min()) > 0
    g = grid_to_dev(d.ds_dout, dev)
    assert_plane_sums(pb.background, g, 3, npdt, "ds_dbackground of the last cell chunks")
    args = pose_args(d, dev)
    got, loss = dpr_amd.raster_residual_pullback_(g, torch.zeros_like(g), *args, scale=1.0, algo="ordered")
    assert_plane_sums(loss, g * g, 3, npdt, "loss of the last cell chunks")
    assert float(loss.min()) > 0
    for b in range(B):
        one = [a if a.shape[0] == s["P"] else a[b:b + 1] for a in args]
        _, l1 = dpr_amd.raster_residual_pullback_(g[..., b:b + 1], torch.zeros_like(g[..., b:b + 1]), *one,
                                                  scale=1.0, algo="ordered")
        assert_same_bits(l1[0], loss[b], f"pose {b} alone: loss")
    assert_same_bits(got.background, pb.background, "residual with target 0 and scale 1: ds_dbackground")


# ------------------------------------------------------------------ A.7 smooth splat: B poses
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 2)])
def test_smooth_poses_across_the_launch_cuts(dev, npdt, tdt, n_in, n_out):
    """ATOMIC forward: k_smooth_fwd_atomic strides the poses over gridDim.y = 65535, fill_background is cut between
    poses.  Pullback: grid_sum's cut, and k_smooth_bwd takes its poses from blockIdx.y (2 blocks of points: 1010
    slices of 65 poses).  Everything against tests/smooth_reference.py in fp64 on the inputs of the working type."""
    s = A_SMOOTH
    B, P, grid = s["B"], s["P"], s["grid"]
    assert B > LAUNCH
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=70 + n_in, dtype=npdt)
    rng = np.random.default_rng(71)
    r = lambda a: np.asarray(a, dtype=npdt).astype(np.float64)
    pts, R, t = r(d.points), r(d.rotations), r(d.translations)
    pts[::25] *= 3.0  # some outside the grid
    pts = r(pts)
    pw, ow_all = r(rng.uniform(0.5, 1.5, size=P)), r(rng.uniform(0.5, 1.5, size=B))
    bg = r(distinct(B, 14))
    assert len(np.unique(bg)) == B
    sel = around_the_cut(B)
    rest = np.ones(B, dtype=bool)
    rest[sel] = False
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    dpts, dR, dt, dbg, dpw = (to(a) for a in (pts, R, t, bg, pw))
    isel, irest = T(np.asarray(sel), dev), T(rest, dev)
    # forward: out_weight is non-zero only on the five poses around the cut
    ow = np.where(rest, 0.0, ow_all)
    out = dpr_amd.raster_smooth(grid, dpts, dR, dt, dbg, to(ow), dpw, algo="atomic")
    assert tuple(out.shape) == grid + (B,) and out.dtype == tdt
    ref = SR.raster_smooth(grid, pts, R[sel], t[sel], bg[sel], ow[sel], pw)
    for i, b in enumerate(sel):
        assert float(np.abs(ref[..., i] - bg[b]).max()) > 0.1
        assert_close(out[..., b], ref[..., i].astype(npdt), smooth_tol(npdt, "out"), f"out[.., {b}]")
    mem = out.permute(2, 1, 0)
    assert mem.is_contiguous()
    assert_planes_equal(mem[irest][None], dbg[irest][None], "a pose of out_weight 0 is not its background")
    # pullback: ds_dout is non-zero only in those five poses; every out_weight is
    gen = torch.Generator(device=dev).manual_seed(72)
    g_mem = torch.zeros((B,) + grid[::-1], dtype=tdt, device=dev)
    g_mem[isel] = torch.randn((len(sel),) + grid[::-1], generator=gen, dtype=tdt, device=dev)
    g = g_mem.permute(2, 1, 0)
    pb = dpr_amd.raster_pullback_smooth_(g, dpts, dR, dt, dbg, to(ow_all), dpw)
    torch.cuda.synchronize()
    want = SR.raster_pullback_smooth(g[..., isel].cpu().numpy().astype(np.float64), pts, R[sel], t[sel], ow_all[sel],
                                     pw)
    assert_close(pb.points, want[0].astype(npdt), smooth_tol(npdt, "points"), "ds_dpoints")
    assert_close(pb.point_weight, want[5].astype(npdt), smooth_tol(npdt, "points"), "ds_dpoint_weight")
    for name, got, e in (("ds_drotation", pb.rotation, want[1]), ("ds_dtranslation", pb.translation, want[2]),
                         ("ds_dout_weight", pb.out_weight, want[4])):
        for i, b in enumerate(sel):
            assert float(np.abs(e[i]).max()) > 0
            assert_close(got[b:b + 1], e[i:i + 1].astype(npdt), smooth_tol(npdt, "pose"), f"{name}[{b}]")
        assert not bool((got[irest] != 0).any()), f"{name}: a pose without sensitivity is not 0"
    assert_plane_sums(pb.background, g, n_out, npdt, "ds_dbackground")
    assert bool((pb.background[isel] != 0).all())


# ------------------------------------------------------------------ A.8 smooth sampling: B poses
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 2)])
def test_sample_smooth_poses_across_the_launch_cuts(dev, npdt, tdt, n_in, n_out):
    """k_sample_smooth_fwd and k_sample_smooth_bwd (ATOMIC) take their poses from blockIdx.y: 2 blocks of points,
    1010 slices of 65 poses, the last of 15, B past 65535.  The image (forward) and ds_dvalues (pullback) are non-zero
    only in the five poses around the cut, so every other column, plane and per-pose sum is exactly 0 and ds_dpoints
    is the reference's over those five.  Against tests/sample_smooth_reference.py in fp64 on the inputs of the working
    type; the pullback writes into NaN-filled buffers.  (The TILED pullback: see the module docstring.)"""
    s = A_SAMPLE_SMOOTH
    B, P, grid = s["B"], s["P"], s["grid"]
    assert B > LAUNCH
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B, grid_n=grid, seed=80 + n_in, dtype=npdt)
    r = lambda a: np.asarray(a, dtype=npdt).astype(np.float64)
    pts, R, t = r(d.points), r(d.rotations), r(d.translations)
    pts[::25] *= 3.0  # some outside the grid
    pts = r(pts)
    sel = around_the_cut(B)
    rest = np.ones(B, dtype=bool)
    rest[sel] = False
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(tdt)
    dpts, dR, dt = (to(a) for a in (pts, R, t))
    isel, irest = T(np.asarray(sel), dev), T(rest, dev)
    gen = torch.Generator(device=dev).manual_seed(81)
    img_mem = torch.zeros((B,) + grid[::-1], dtype=tdt, device=dev)
    img_mem[isel] = torch.randn((len(sel),) + grid[::-1], generator=gen, dtype=tdt, device=dev)
    img = img_mem.permute(2, 1, 0)
    image = img[..., isel].cpu().numpy().astype(np.float64)
    # forward
    v = dpr_amd.sample_smooth(img, dpts, dR, dt)
    assert tuple(v.shape) == (P, B) and v.dtype == tdt and v.t().is_contiguous()
    ref = SSR.sample_smooth(image, pts, R[sel], t[sel])
    for i, b in enumerate(sel):
        assert float(np.abs(ref[:, i]).max()) > 0.1
        assert_close(v[:, b], ref[:, i].astype(npdt), smooth_tol(npdt, "points"), f"values[:, {b}]")
    assert not bool((v.t()[irest] != 0).any()), "the column of a zero image is not 0"
    # pullback
    dv_mem = torch.zeros((B, P), dtype=tdt, device=dev)
    dv_mem[isel] = torch.randn((len(sel), P), generator=gen, dtype=tdt, device=dev)
    nan = float("nan")
    bufs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, tdt, dev).fill_(nan),
                ds_dpoints=torch.full((P, n_in), nan, dtype=tdt, device=dev),
                ds_drotation=torch.full((B, n_in, n_out), nan, dtype=tdt, device=dev).transpose(1, 2),
                ds_dtranslation=torch.full((B, n_out), nan, dtype=tdt, device=dev))
    pb = dpr_amd.sample_smooth_pullback_(dv_mem.t(), img, dpts, dR, dt, algo="atomic", **bufs)
    torch.cuda.synchronize()
    assert pb.image is bufs["ds_dimage"] and pb.points is bufs["ds_dpoints"]
    want = SSR.sample_smooth_pullback(dv_mem[isel].t().cpu().numpy().astype(np.float64), image, pts, R[sel], t[sel])
    assert_close(pb.points, want[1].astype(npdt), smooth_tol(npdt, "points"), "ds_dpoints")
    for name, kind, got, e in (("ds_dimage", "out", pb.image.permute(2, 0, 1), np.moveaxis(want[0], -1, 0)),
                               ("ds_drotation", "pose", pb.rotation, want[2]),
                               ("ds_dtranslation", "pose", pb.translation, want[3])):
        for i, b in enumerate(sel):
            assert float(np.abs(e[i]).max()) > 0
            assert_close(got[b], e[i].astype(npdt), smooth_tol(npdt, kind), f"{name}[{b}]")
        assert not bool((got[irest] != 0).any()), f"{name}: a pose without sensitivity is not 0"


# =================================================================== Part B: a whole plane past element 2^32
def host_plane(t):
    """A (n, n, n) plane of a grid-layout tensor -> numpy"""
    return t.cpu().numpy()


def assert_planes_equal(mem, values, what):
    """mem[i] (one contiguous block of planes each) == values[i] broadcast, block by block on the device."""
    for i in range(mem.shape[0]):
        v = values[i].reshape(values[i].shape + (1,) * (mem.ndim - 1 - values[i].ndim))
        assert bool((mem[i] == v).all()), f"{what}: block {i}"


def cloud_f32(rng, P, n_in=3):
    return (0.4 * rng.standard_normal(size=(P, n_in))).astype(F32)


def poses_f32(rng, B, n_out=3):
    R = D.random_rotations(rng, B)[:, :n_out, :].astype(F32)
    return R, (0.1 * rng.normal(size=(B, n_out))).astype(F32)


def only_first_and_last(values):
    out = np.zeros_like(values)
    out[0], out[-1] = values[0], values[-1]
    return out


# ------------------------------------------------------------------ B.1 channels
@gpu
def test_channels_planes_past_2_pow_32(oracle, dev):
    """16 channels x 17 poses of 256^3: planes 256 .. 271 are pose 16.  TILED and ATOMIC forward, ATOMIC pullback."""
    s = B_CHANNELS
    C, B, grid, P = s["C"], s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * C * G >= 2 ** 32  # every plane of the last pose lies at or past element 2^32
    rng = np.random.default_rng(41)
    pts = cloud_f32(rng, P)
    R, t = poses_f32(rng, B)
    pw = (rng.uniform(0.2, 1.0, size=(P, C)) * (1.0 + np.arange(C))).astype(F32)
    bg = distinct(B * C, 4).reshape(B, C).astype(F32)
    ow = only_first_and_last(np.linspace(0.5, 1.5, B).astype(F32))  # the middle poses: their background exactly
    dpts, dR, dt, dpw, dbg = (T(a, dev) for a in (pts, R, t, pw, bg))
    for algo in ("tiled", "atomic"):
        out = dpr_amd.raster_channels(grid, dpts, dR, dt, dpw, dbg, T(ow, dev), algo=algo)
        torch.cuda.synchronize()
        for b, chans in ((last, range(C)), (0, (0, C - 1))):
            for c in chans:
                ref = oracle.raster(grid, pts, R[b:b + 1], t[b:b + 1], bg[b, c:c + 1], ow[b:b + 1], pw[:, c],
                                    dtype=F32)[..., 0]
                assert_close(out[..., c, b], ref, channels_tol(F32, "out"), f"{algo}: pose {b} channel {c}")
        mem = out.permute(4, 3, 2, 1, 0)
        assert mem.is_contiguous()
        assert_planes_equal(mem[1:last], dbg[1:last], f"{algo}: a middle pose is not its background")
        del out, mem
        torch.cuda.empty_cache()
    # pullback: ds_dout is zero except in pose 16
    gen = torch.Generator(device=dev).manual_seed(42)
    g_mem = torch.zeros((B, C) + grid, dtype=torch.float32, device=dev)
    g_mem[last].normal_(generator=gen)
    g = g_mem.permute(4, 3, 2, 1, 0)
    ow = np.linspace(0.5, 1.5, B).astype(F32)
    pb = dpr_amd.raster_pullback_channels_(g, dpts, dR, dt, dpw, dbg, T(ow, dev), algo="atomic")
    torch.cuda.synchronize()
    sums = None
    for c in range(C):
        r = oracle.raster_pullback(host_plane(g[..., c, last])[..., None], pts, R[last:], t[last:], ow[last:],
                                   pw[:, c], dtype=F32)
        assert_close(pb.point_weight[:, c], r.point_weight, channels_tol(F32, "points"), f"ds_dpoint_weight[:, {c}]")
        assert_close(pb.background[last, c:c + 1], r.background, channels_tol(F32, "pose"), f"ds_dbackground[{c}]")
        parts = [np.asarray(x, np.float64) for x in (r.points, r.rotation[0], r.translation[0], r.out_weight)]
        sums = parts if sums is None else [a + x for a, x in zip(sums, parts)]
    assert_close(pb.points, sums[0], channels_tol(F32, "points"), "ds_dpoints")
    assert_close(pb.rotation[last], sums[1], channels_tol(F32, "pose"), "ds_drotation[last]")
    assert_close(pb.translation[last], sums[2], channels_tol(F32, "pose"), "ds_dtranslation[last]")
    assert_close(pb.out_weight[last:], sums[3], channels_tol(F32, "pose"), "ds_dout_weight[last]")
    for name in ("rotation", "translation", "out_weight", "background"):
        assert not bool((getattr(pb, name)[:last] != 0).any()), f"ds_d{name} of the poses before the last is not 0"
    del g, g_mem, pb
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.2 JVP
@gpu
def test_jvp_planes_past_2_pow_32(dev):
    """16 tangents x 17 poses of 256^3: planes 256 .. 271 are pose 16.  TILED and ATOMIC, every tangent given (the
    tangents of the points and the point weights are read at k * P * NI and k * P)."""
    s = B_JVP
    K, B, grid, P = s["K"], s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * K * G >= 2 ** 32
    assert (K - 1) * P * 3 < 2 ** 32  # (the tangent offsets stay far below: see the module docstring)
    rng = np.random.default_rng(43)
    r = lambda a: np.asarray(a, dtype=F32).astype(np.float64)
    pts = r(cloud_f32(rng, P))
    R, t = (r(a) for a in poses_f32(rng, B))
    pw = r(rng.uniform(0.5, 2.0, size=P))
    ow = r(only_first_and_last(rng.uniform(0.5, 2.0, size=B)))
    tan = {k: r(v) for k, v in random_tangents(rng, K, P, B, 3, 3).items()}
    tan["out_weight"][:, 1:last] = 0.0  # the middle poses deposit nothing: their planes are background_dot exactly
    tan["background"] = r(distinct(K * B, 4).reshape(K, B))
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(torch.float32)
    kw = {k + "_dot": to(v) for k, v in tan.items()}
    per_pose = ("rotation", "translation", "background", "out_weight")
    refs = {}
    for b, nk in ((last, K), (0, 2)):  # the last pose: every tangent; pose 0: the first two
        sub = {k: (v[:nk, b:b + 1] if k in per_pose else v[:nk]) for k, v in tan.items()}
        refs[b] = jvp_reference(grid, pts, R[b:b + 1], t[b:b + 1], ow[b:b + 1], pw, sub, nk, cell_dtype=F32)
    for algo in ("tiled", "atomic"):
        out = dpr_amd.raster_jvp(grid, to(pts), to(R), to(t), None, to(ow), to(pw), **kw, tangents=K, algo=algo)
        torch.cuda.synchronize()
        assert tuple(out.shape) == grid + (K, B)
        for b, ref in refs.items():
            for k in range(ref.shape[-2]):
                assert_close(out[..., k, b], ref[..., k, 0], jvp_tol(F32), f"{algo}: pose {b} tangent {k}")
        mem = out.permute(4, 3, 2, 1, 0)
        assert mem.is_contiguous()
        assert_planes_equal(mem[1:last], kw["background_dot"].t()[1:last], f"{algo}: a middle pose")
        del out, mem
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.3 sampling
def oracle_sample(oracle, image_plane, pts, R, t, b, dv=None):
    return oracle.raster_pullback(image_plane[..., None], pts, R[b:b + 1], t[b:b + 1], np.ones(1, F32), dv, dtype=F32)


@gpu
def test_sample_image_past_2_pow_32(oracle, dev):
    """257 images of 256^3: image 256 starts at element 2^32.  Forward; pullback on ATOMIC and TILED with ds_dvalues
    zero except for poses 0 and 256."""
    s = B_SAMPLE_IMAGE
    B, grid, P = s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * G >= 2 ** 32
    rng = np.random.default_rng(44)
    pts = cloud_f32(rng, P)
    R, t = poses_f32(rng, B)
    dv = only_first_and_last(rng.standard_normal(size=(B, P)).astype(F32))
    gen = torch.Generator(device=dev).manual_seed(44)
    img = torch.randn((B,) + grid, generator=gen, device=dev).permute(3, 2, 1, 0)
    dpts, dR, dt = T(pts, dev), T(R, dev), T(t, dev)
    v = dpr_amd.sample(img, dpts, dR, dt)
    torch.cuda.synchronize()
    planes = {b: host_plane(img[..., b]) for b in (0, last)}
    want = {b: oracle_sample(oracle, planes[b], pts, R, t, b, dv[b]) for b in (0, last)}
    for b in (last, 0):
        assert_close(v[:, b], oracle_sample(oracle, planes[b], pts, R, t, b).point_weight, sample_tol(F32, "out"),
                     f"values[:, {b}]")
    del v
    d_img = dpr_amd.empty_grid(grid, B, torch.float32, dev)
    for algo in ("atomic", "tiled"):
        d_img.fill_(float("nan"))
        pb = dpr_amd.sample_pullback_(T(dv, dev).t(), img, dpts, dR, dt, ds_dimage=d_img, algo=algo)
        torch.cuda.synchronize()
        assert pb.image is d_img
        for b in (last, 0):
            ref = oracle.raster(grid, pts, R[b:b + 1], t[b:b + 1], None, None, dv[b], dtype=F32)[..., 0]
            assert_close(pb.image[..., b], ref, sample_tol(F32, "out"), f"{algo}: ds_dimage[.., {b}]")
            assert_close(pb.rotation[b], want[b].rotation[0], sample_tol(F32, "pose"), f"{algo}: ds_drotation[{b}]")
            assert_close(pb.translation[b], want[b].translation[0], sample_tol(F32, "pose"),
                         f"{algo}: ds_dtranslation[{b}]")
        assert_close(pb.points, np.asarray(want[0].points, np.float64) + want[last].points, sample_tol(F32, "points"),
                     f"{algo}: ds_dpoints")
        mem = d_img.permute(3, 2, 1, 0)
        assert_planes_equal(mem[1:last], torch.zeros(B, device=dev)[1:last], f"{algo}: ds_dimage of a middle pose")
        assert not bool((pb.rotation[1:last] != 0).any()) and not bool((pb.translation[1:last] != 0).any())
    del img, d_img, pb, mem
    torch.cuda.empty_cache()


@gpu
def test_sample_values_past_2_pow_32(oracle, dev):
    """2^24 points x 257 poses on 16^3 images: column 256 of `values` starts at element 2^32."""
    s = B_SAMPLE_VALUES
    B, grid, P = s["B"], s["grid"], s["P"]
    last = B - 1
    assert last * P >= 2 ** 32
    rng = np.random.default_rng(45)
    R, t = poses_f32(rng, B)
    gen = torch.Generator(device=dev).manual_seed(45)
    dpts = 0.4 * torch.randn((P, 3), generator=gen, device=dev)
    img_mem = torch.zeros((B,) + grid, device=dev)  # the middle images are zero: their columns must be
    img_mem[0].normal_(generator=gen)
    img_mem[last].normal_(generator=gen)
    img = img_mem.permute(3, 2, 1, 0)
    dR, dt = T(R, dev), T(t, dev)
    v = dpr_amd.sample(img, dpts, dR, dt)
    torch.cuda.synchronize()
    assert tuple(v.shape) == (P, B) and v.t().is_contiguous()
    sub = T(rng.choice(P, 100_000, replace=False), dev)
    spts = dpts[sub].cpu().numpy()
    for b in (last, 0):
        ref = oracle_sample(oracle, host_plane(img[..., b]), spts, R, t, b).point_weight
        assert_close(v[sub, b], ref, sample_tol(F32, "out"), f"values[subsample, {b}]")
        # the whole column: the same kernel on the pose alone, value by value (no sum is involved)
        alone = dpr_amd.sample(img[..., b:b + 1], dpts, dR[b:b + 1], dt[b:b + 1])
        assert torch.equal(v[:, b], alone[:, 0]), f"values[:, {b}] is not the column of the pose alone"
        del alone
    assert_planes_equal(v.t()[1:last], torch.zeros(B, device=dev)[1:last], "the column of a zero image")
    del v
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.4 per-pose clouds
@gpu
def test_clouds_out_past_2_pow_32(oracle, dev):
    """257 clouds of 20 000 points on 256^3: plane 256 starts at element 2^32.  TILED, ATOMIC and CHUNKED (2048 tiles
    a pose: not AUTO's choice, but nothing is refused), forward and pullback (ds_dout zero except for poses 0 and
    256)."""
    s = B_CLOUDS_OUT
    B, grid, P = s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * G >= 2 ** 32
    rng = np.random.default_rng(46)
    pts = ((0.15 + 0.4 * rng.uniform(size=(B, 1, 1))) * rng.standard_normal(size=(B, P, 3))).astype(F32)
    R, t = poses_f32(rng, B)
    pw = rng.uniform(0.5, 1.5, size=(B, P)).astype(F32)
    bg = distinct(B, 6).astype(F32)
    ow_all = rng.uniform(1, 10, size=B).astype(F32)
    ow = only_first_and_last(ow_all)
    dpts, dR, dt, dpw, dbg = (T(a, dev) for a in (pts, R, t, pw, bg))
    for algo in ("tiled", "atomic", "chunked"):
        out = dpr_amd.raster_clouds(grid, dpts, dR, dt, dbg, T(ow, dev), dpw, algo=algo)
        torch.cuda.synchronize()
        for b in (last, 0):
            ref = oracle.raster(grid, pts[b], R[b:b + 1], t[b:b + 1], bg[b:b + 1], ow[b:b + 1], pw[b], dtype=F32)
            assert_close(out[..., b], ref[..., 0], clouds_tol(F32, "out"), f"{algo}: out[.., {b}]")
        assert_planes_equal(out.permute(3, 2, 1, 0)[1:last], dbg[1:last], f"{algo}: a middle pose")
        del out
        torch.cuda.empty_cache()
    gen = torch.Generator(device=dev).manual_seed(46)
    g_mem = torch.zeros((B,) + grid, device=dev)
    g_mem[0].normal_(generator=gen)
    g_mem[last].normal_(generator=gen)
    g = g_mem.permute(3, 2, 1, 0)
    want = {b: oracle.raster_pullback(host_plane(g[..., b])[..., None], pts[b], R[b:b + 1], t[b:b + 1],
                                      ow_all[b:b + 1], pw[b], dtype=F32) for b in (0, last)}
    for algo in ("tiled", "atomic", "chunked"):
        pb = dpr_amd.raster_pullback_clouds_(g, dpts, dR, dt, dbg, T(ow_all, dev), dpw, algo=algo)
        torch.cuda.synchronize()
        for b, r in want.items():
            assert_close(pb.points[b], r.points, clouds_tol(F32, "points"), f"{algo}: ds_dpoints[{b}]")
            assert_close(pb.point_weight[b], r.point_weight, clouds_tol(F32, "points"),
                         f"{algo}: ds_dpoint_weight[{b}]")
            assert_close(pb.rotation[b], r.rotation[0], clouds_tol(F32, "pose"), f"{algo}: ds_drotation[{b}]")
            assert_close(pb.translation[b], r.translation[0], clouds_tol(F32, "pose"), f"{algo}: ds_dtranslation[{b}]")
            assert_close(pb.background[b:b + 1], r.background, clouds_tol(F32, "pose"), f"{algo}: ds_dbackground[{b}]")
            assert_close(pb.out_weight[b:b + 1], r.out_weight, clouds_tol(F32, "pose"), f"{algo}: ds_dout_weight[{b}]")
        for name in ("points", "point_weight", "rotation", "translation", "background", "out_weight"):
            assert not bool((getattr(pb, name)[1:last] != 0).any()), f"{algo}: ds_d{name} of a middle pose is not 0"
    del g, g_mem, pb
    torch.cuda.empty_cache()


@gpu
def test_clouds_points_past_2_pow_32(oracle, dev):
    """343 clouds of 2^22 3-D points on 16^2: cloud 342 starts at element 342 * 2^22 * 3 > 2^32 of `points` and of
    ds_dpoints.  ATOMIC and CHUNKED, forward and pullback; no point weights (two more arrays of 5.8 GB)."""
    s = B_CLOUDS_POINTS
    B, grid, P, NI = s["B"], s["grid"], s["P"], s["n_in"]
    last = B - 1
    assert last * P * NI >= 2 ** 32
    rng = np.random.default_rng(47)
    R, t = poses_f32(rng, B, 2)
    bg = distinct(B, 6).astype(F32)
    ow_all = rng.uniform(1, 10, size=B).astype(F32)
    ow = only_first_and_last(ow_all)
    ds = np.asfortranarray(rng.standard_normal(size=grid + (B,)).astype(F32))
    gen = torch.Generator(device=dev).manual_seed(47)
    dpts = torch.randn((B, P, NI), generator=gen, device=dev)
    dpts *= 0.4
    dR, dt, dbg = T(R, dev), T(t, dev), T(bg, dev)
    g = dpr_amd.to_grid_layout(T(ds, dev))
    ends = {b: dpts[b].cpu().numpy() for b in (0, last)}
    want = {b: oracle.raster_pullback(ds[..., b:b + 1], ends[b], R[b:b + 1], t[b:b + 1], ow_all[b:b + 1], None,
                                      dtype=F32, threaded=True) for b in (0, last)}
    # The per-pose sums run over 2^22 points: the serial fp32 oracle's own rounding reaches the tolerance there
    # (3e-4 .. 3e-3 of ds_dtranslation / ds_dout_weight against its fp64 run), so they are compared with the fp64
    # oracle of the same fp32 inputs.  ds_dpoints needs the fp32 cell choices (its gradient jumps at a cell face).
    r64 = lambda a: np.asarray(a, np.float64)
    want64 = {b: oracle.raster_pullback(r64(ds[..., b:b + 1]), r64(ends[b]), r64(R[b:b + 1]), r64(t[b:b + 1]),
                                        r64(ow_all[b:b + 1]), None, dtype=np.float64, threaded=True)
              for b in (0, last)}
    d_pts = torch.empty((B, P, NI), device=dev)
    for algo in ("atomic", "chunked"):
        out = dpr_amd.raster_clouds(grid, dpts, dR, dt, dbg, T(ow, dev), None, algo=algo)
        torch.cuda.synchronize()
        for b in (last, 0):
            ref = oracle.raster(grid, ends[b], R[b:b + 1], t[b:b + 1], bg[b:b + 1], ow[b:b + 1], None, dtype=F32,
                                threaded=True)
            assert_close(out[..., b], ref[..., 0], clouds_tol(F32, "out"), f"{algo}: out[.., {b}]")
        assert_planes_equal(out.permute(2, 1, 0)[1:last], dbg[1:last], f"{algo}: a middle pose")
        d_pts.fill_(float("nan"))
        pb = dpr_amd.raster_pullback_clouds_(g, dpts, dR, dt, dbg, T(ow_all, dev), None, ds_dpoints=d_pts, algo=algo,
                                             point_weight_grad=False)
        torch.cuda.synchronize()
        assert pb.points is d_pts and pb.point_weight is None
        for b, r in want64.items():
            assert_close(pb.points[b], want[b].points, clouds_tol(F32, "points"), f"{algo}: ds_dpoints[{b}]")
            assert_close(pb.rotation[b], r.rotation[0], clouds_tol(F32, "pose"), f"{algo}: ds_drotation[{b}]")
            assert_close(pb.translation[b], r.translation[0], clouds_tol(F32, "pose"), f"{algo}: ds_dtranslation[{b}]")
            assert_close(pb.out_weight[b:b + 1], r.out_weight, clouds_tol(F32, "pose"), f"{algo}: ds_dout_weight[{b}]")
        assert_plane_sums(pb.background, g, 2, F32, f"{algo}: ds_dbackground")
        assert not bool(torch.isnan(d_pts.view(-1)[:: 4099]).any()), f"{algo}: ds_dpoints not overwritten"
        del out, pb
    del dpts, d_pts
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.5 ORDERED
@gpu
def test_ordered_pose_past_2_pow_32(oracle, dev):
    """257 poses of 256^3: pose 256 starts at element 2^32.  The forward plane and, with ds_dout zero except in pose
    256, the point gradients against the serial oracle, bit for bit; the pose's sums equal to the pose alone."""
    s = B_ORDERED
    B, grid, P = s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * G >= 2 ** 32
    rng = np.random.default_rng(48)
    pts = cloud_f32(rng, P)
    R, t = poses_f32(rng, B)
    pw = rng.uniform(0.5, 1.5, size=P).astype(F32)
    bg = distinct(B, 6).astype(F32)
    ow_all = rng.uniform(1, 10, size=B).astype(F32)
    ow = only_first_and_last(ow_all)
    dpts, dR, dt, dpw, dbg = (T(a, dev) for a in (pts, R, t, pw, bg))
    out = dpr_amd.raster(grid, dpts, dR, dt, dbg, T(ow, dev), dpw, algo="ordered")
    torch.cuda.synchronize()
    for b in (last, 0):
        ref = oracle.raster(grid, pts, R[b:b + 1], t[b:b + 1], bg[b:b + 1], ow[b:b + 1], pw, dtype=F32)[..., 0]
        assert_same_bits(out[..., b], np.ascontiguousarray(ref), f"out[.., {b}]")
    assert_planes_equal(out.permute(3, 2, 1, 0)[1:last], dbg[1:last], "a middle pose")
    del out
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev).manual_seed(48)
    g_mem = torch.zeros((B,) + grid, device=dev)
    g_mem[last].normal_(generator=gen)
    g = g_mem.permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_(g, dpts, dR, dt, dbg, T(ow_all, dev), dpw, algo="ordered")
    ref = oracle.raster_pullback(host_plane(g[..., last])[..., None], pts, R[last:], t[last:], ow_all[last:], pw,
                                 dtype=F32)
    assert_same_bits(pb.points, ref.points, "ds_dpoints")
    assert_same_bits(pb.point_weight, ref.point_weight, "ds_dpoint_weight")
    alone = dpr_amd.raster_pullback_(g[..., last:], dpts, dR[last:], dt[last:], dbg[last:], T(ow_all[last:], dev),
                                     dpw, algo="ordered")
    torch.cuda.synchronize()
    for name in POSE_FIELDS:
        assert_same_bits(getattr(alone, name)[0], getattr(pb, name)[last], f"pose {last} alone: {name}")
        assert_close(getattr(pb, name)[last:], getattr(ref, name), ordered_tol(F32, "pose"), name)
        assert not bool((getattr(pb, name)[:last] != 0).any()), f"ds_d{name} of the poses before the last is not 0"
    del g, g_mem, pb, alone
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.6 smooth splat
@gpu
def test_smooth_pose_past_2_pow_32(dev):
    """257 poses of 256^3: pose 256 starts at element 2^32.  ATOMIC and TILED forward with out_weight zero except
    for poses 0 and 256; the pullback with ds_dout zero except in pose 256.  Against tests/smooth_reference.py in
    fp64 on the fp32 inputs."""
    s = B_SMOOTH
    B, grid, P = s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * G >= 2 ** 32
    rng = np.random.default_rng(49)
    r64 = lambda a: np.asarray(a, np.float64)
    pts = cloud_f32(rng, P)
    R, t = poses_f32(rng, B)
    pw = rng.uniform(0.5, 1.5, size=P).astype(F32)
    bg = distinct(B, 6).astype(F32)
    ow_all = rng.uniform(0.5, 1.5, size=B).astype(F32)
    ow = only_first_and_last(ow_all)
    dpts, dR, dt, dpw, dbg = (T(a, dev) for a in (pts, R, t, pw, bg))
    refs = {b: SR.raster_smooth(grid, r64(pts), r64(R[b:b + 1]), r64(t[b:b + 1]), r64(bg[b:b + 1]), r64(ow[b:b + 1]),
                                r64(pw))[..., 0].astype(F32) for b in (0, last)}
    for algo in ("atomic", "tiled"):
        out = dpr_amd.raster_smooth(grid, dpts, dR, dt, dbg, T(ow, dev), dpw, algo=algo)
        torch.cuda.synchronize()
        for b in (last, 0):
            assert_close(out[..., b], refs[b], smooth_tol(F32, "out"), f"{algo}: out[.., {b}]")
        assert_planes_equal(out.permute(3, 2, 1, 0)[1:last], dbg[1:last], f"{algo}: a middle pose")
        del out
        torch.cuda.empty_cache()
    del refs
    gen = torch.Generator(device=dev).manual_seed(49)
    g_mem = torch.zeros((B,) + grid, device=dev)
    g_mem[last].normal_(generator=gen)
    g = g_mem.permute(3, 2, 1, 0)
    pb = dpr_amd.raster_pullback_smooth_(g, dpts, dR, dt, dbg, T(ow_all, dev), dpw)
    torch.cuda.synchronize()
    ref = SR.raster_pullback_smooth(host_plane(g[..., last])[..., None], r64(pts), r64(R[last:]), r64(t[last:]),
                                    r64(ow_all[last:]), r64(pw))
    assert_close(pb.points, ref[0], smooth_tol(F32, "points"), "ds_dpoints")
    assert_close(pb.point_weight, ref[5], smooth_tol(F32, "points"), "ds_dpoint_weight")
    for name, got, e in (("rotation", pb.rotation, ref[1]), ("translation", pb.translation, ref[2]),
                         ("background", pb.background, ref[3]), ("out_weight", pb.out_weight, ref[4])):
        assert_close(got[last:], e, smooth_tol(F32, "pose"), f"ds_d{name}[{last}]")
        assert not bool((got[:last] != 0).any()), f"ds_d{name} of the poses before the last is not 0"
    del g, g_mem, pb
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B.7 smooth sampling
def ssr_pose(image_plane, pts, R, t, b, dv=None):
    """SSR in fp64 on fp32 inputs for pose b alone: the values, or with dv (P,) the pullback"""
    r64 = lambda a: np.asarray(a, np.float64)
    a = (r64(image_plane)[..., None], r64(pts), r64(R[b:b + 1]), r64(t[b:b + 1]))
    return SSR.sample_smooth(*a)[:, 0] if dv is None else SSR.sample_smooth_pullback(r64(dv)[:, None], *a)


@gpu
def test_sample_smooth_image_past_2_pow_32(dev):
    """257 images of 256^3: image 256 starts at element 2^32.  Forward with the images zero except 0 and 256;
    pullback on ATOMIC and TILED with ds_dvalues zero except for poses 0 and 256, into a NaN-filled ds_dimage."""
    s = B_SAMPLE_SMOOTH_IMAGE
    B, grid, P = s["B"], s["grid"], s["P"]
    G, last = cells(grid), B - 1
    assert last * G >= 2 ** 32
    rng = np.random.default_rng(54)
    pts = cloud_f32(rng, P)
    R, t = poses_f32(rng, B)
    dv = only_first_and_last(rng.standard_normal(size=(B, P)).astype(F32))
    gen = torch.Generator(device=dev).manual_seed(54)
    img_mem = torch.zeros((B,) + grid, device=dev)
    img_mem[0].normal_(generator=gen)
    img_mem[last].normal_(generator=gen)
    img = img_mem.permute(3, 2, 1, 0)
    dpts, dR, dt = T(pts, dev), T(R, dev), T(t, dev)
    v = dpr_amd.sample_smooth(img, dpts, dR, dt)
    torch.cuda.synchronize()
    planes = {b: host_plane(img[..., b]) for b in (0, last)}
    for b in (last, 0):
        assert_close(v[:, b], ssr_pose(planes[b], pts, R, t, b), smooth_tol(F32, "points"), f"values[:, {b}]")
    assert not bool((v.t()[1:last] != 0).any()), "the column of a zero image is not 0"
    del v
    want = {b: ssr_pose(planes[b], pts, R, t, b, dv[b]) for b in (0, last)}
    d_img = dpr_amd.empty_grid(grid, B, torch.float32, dev)
    for algo in ("atomic", "tiled"):
        d_img.fill_(float("nan"))
        pb = dpr_amd.sample_smooth_pullback_(T(dv, dev).t(), img, dpts, dR, dt, ds_dimage=d_img, algo=algo)
        torch.cuda.synchronize()
        assert pb.image is d_img
        for b in (last, 0):
            ref = want[b]
            assert_close(pb.image[..., b], ref[0][..., 0].astype(F32), smooth_tol(F32, "out"),
                         f"{algo}: ds_dimage[.., {b}]")
            assert_close(pb.rotation[b], ref[2][0], smooth_tol(F32, "pose"), f"{algo}: ds_drotation[{b}]")
            assert_close(pb.translation[b], ref[3][0], smooth_tol(F32, "pose"), f"{algo}: ds_dtranslation[{b}]")
        assert_close(pb.points, want[0][1] + want[last][1], smooth_tol(F32, "points"), f"{algo}: ds_dpoints")
        mem = d_img.permute(3, 2, 1, 0)
        assert_planes_equal(mem[1:last], torch.zeros(B, device=dev)[1:last], f"{algo}: ds_dimage of a middle pose")
        assert not bool((pb.rotation[1:last] != 0).any()) and not bool((pb.translation[1:last] != 0).any())
    del img, img_mem, d_img, pb, mem
    torch.cuda.empty_cache()


@gpu
def test_sample_smooth_values_past_2_pow_32(dev):
    """2^24 points x 257 poses on 16^3 images: column 256 of `values` and of ds_dvalues starts at element 2^32.
    Forward with the images zero except 0 and 256; then, `values` freed, the pullback on both algorithms with
    ds_dvalues zero except in column 256 (there: at 100 000 points drawn from all 2^24, see the module docstring).
    The cloud is wide (2 N(0, 1): one point in thirteen is accepted under a pose): the tiled planes of 2^24 accepted
    points on the four tiles of 16^3, 257 times, and the image atomics of as many, would take 17 s."""
    s = B_SAMPLE_SMOOTH_VALUES
    B, grid, P = s["B"], s["grid"], s["P"]
    last = B - 1
    assert last * P >= 2 ** 32
    rng = np.random.default_rng(55)
    R, t = poses_f32(rng, B)
    gen = torch.Generator(device=dev).manual_seed(55)
    dpts = 2.0 * torch.randn((P, 3), generator=gen, device=dev)
    img_mem = torch.zeros((B,) + grid, device=dev)  # the middle images are zero: their columns must be
    img_mem[0].normal_(generator=gen)
    img_mem[last].normal_(generator=gen)
    img = img_mem.permute(3, 2, 1, 0)
    dR, dt = T(R, dev), T(t, dev)
    v = dpr_amd.sample_smooth(img, dpts, dR, dt)
    torch.cuda.synchronize()
    assert tuple(v.shape) == (P, B) and v.t().is_contiguous()
    chosen = np.sort(rng.choice(P, 100_000, replace=False))
    assert chosen[0] < P // 100 and chosen[-1] > P - P // 100
    sub = T(chosen, dev)
    spts = dpts[sub].cpu().numpy()
    for b in (last, 0):
        ref = ssr_pose(host_plane(img[..., b]), spts, R, t, b)
        assert 5000 < np.count_nonzero(ref) < 12_000  # (accepted and rejected points in the subsample)
        assert_close(v[sub, b], ref, smooth_tol(F32, "points"), f"values[subsample, {b}]")
        # the whole column: the same kernel on the pose alone, value by value (no sum is involved)
        alone = dpr_amd.sample_smooth(img[..., b:b + 1], dpts, dR[b:b + 1], dt[b:b + 1])
        assert torch.equal(v[:, b], alone[:, 0]), f"values[:, {b}] is not the column of the pose alone"
        del alone
    assert_planes_equal(v.t()[1:last], torch.zeros(B, device=dev)[1:last], "the column of a zero image")
    del v
    torch.cuda.empty_cache()
    # pullback
    dv_mem = torch.zeros((B, P), device=dev)
    dv_mem[last, sub] = torch.randn(len(chosen), generator=gen, device=dev)
    ref = ssr_pose(host_plane(img[..., last]), spts, R, t, last, dv_mem[last, sub].cpu().numpy())
    assert np.count_nonzero(ref[1].any(axis=1)) > 5000
    others = torch.ones(P, dtype=torch.bool, device=dev)
    others[sub] = False
    for algo in ("atomic", "tiled"):
        d_img = dpr_amd.empty_grid(grid, B, torch.float32, dev).fill_(float("nan"))
        d_pts = torch.full((P, 3), float("nan"), device=dev)
        pb = dpr_amd.sample_smooth_pullback_(dv_mem.t(), img, dpts, dR, dt, ds_dimage=d_img, ds_dpoints=d_pts,
                                             algo=algo)
        torch.cuda.synchronize()
        assert pb.image is d_img and pb.points is d_pts
        assert_close(pb.image[..., last], ref[0][..., 0].astype(F32), smooth_tol(F32, "out"),
                     f"{algo}: ds_dimage[.., {last}]")
        assert_close(pb.rotation[last], ref[2][0], smooth_tol(F32, "pose"), f"{algo}: ds_drotation[{last}]")
        assert_close(pb.translation[last], ref[3][0], smooth_tol(F32, "pose"), f"{algo}: ds_dtranslation[{last}]")
        assert_close(pb.points[sub], ref[1], smooth_tol(F32, "points"), f"{algo}: ds_dpoints[subsample]")
        assert not bool((pb.points[others] != 0).any()), f"{algo}: ds_dpoints of a point without sensitivity is not 0"
        assert not bool((d_img.permute(3, 2, 1, 0)[:last] != 0).any()), f"{algo}: ds_dimage before pose {last} is not 0"
        assert not bool((pb.rotation[:last] != 0).any()) and not bool((pb.translation[:last] != 0).any()), \
            f"{algo}: a per-pose sum before pose {last} is not 0"
        del pb, d_img, d_pts
    del dv_mem, img, img_mem, dpts
    torch.cuda.empty_cache()


# =================================================================== the CPU side
def test_shapes_cross_the_limit_they_name_and_no_other():
    """Recomputed from DPR_ORDERED_POINT_CHUNK / DPR_ORDERED_CELL_CHUNK of include/dpr.h and the literals 65535,
    2^20 and 256 of the drivers: a later change of a constant must not move a test back inside the first launch."""
    GB = 2 ** 30
    # Part A: one limit each, tiny planes (at most 1 MB in fp64), small arrays
    for s in (A_CHANNELS_PLANES, A_CHANNELS_POSES, A_JVP_PLANES, A_JVP_POSES, A_CLOUDS, A_ORDERED, A_ORD_POINTS,
              A_SMOOTH, A_SAMPLE_SMOOTH):
        assert cells(s["grid"]) * 8 <= 2 ** 20, s
        assert cells(s["grid"]) * s["B"] * s.get("C", s.get("K", 1)) < 2 ** 31, s  # no offset near 2^32
    for s, per_pose in ((A_CHANNELS_PLANES, "C"), (A_JVP_PLANES, "K")):
        assert s["B"] <= LAUNCH < s["B"] * s[per_pose] <= 2 * LAUNCH and s[per_pose] <= 16
        assert LAUNCH % s[per_pose] != 0  # the cut falls inside a pose
    for s, per_pose in ((A_CHANNELS_POSES, "C"), (A_JVP_POSES, "K")):
        assert LAUNCH < s["B"] <= 2 * LAUNCH and s[per_pose] <= 16
    s = A_CLOUDS
    assert LAUNCH < s["B"] <= 2 * LAUNCH
    assert s["grid"][0] <= 128 and s["grid"][1] <= 78 and s["P"] <= 2048  # one tile, one slice: only b0 varies
    s = A_ORDERED
    NV = len(s["grid"]) * s["n_in"] + len(s["grid"]) + 1
    assert LAUNCH < s["B"] <= 2 * LAUNCH and REDUCE_BLOCKS < s["B"] * (NV + 2) <= 2 * REDUCE_BLOCKS
    assert -(-s["P"] // POINT_CHUNK) <= STAGE and -(-cells(s["grid"]) // CELL_CHUNK) <= STAGE
    s = A_ORD_POINTS
    assert STAGE < -(-s["P"] // POINT_CHUNK) <= 2 * STAGE and -(-cells(s["grid"]) // CELL_CHUNK) <= STAGE
    assert s["P"] % POINT_CHUNK != 0 and s["P"] - STAGE * POINT_CHUNK > POINT_CHUNK  # chunks 256 and 257, one partial
    assert s["B"] <= LAUNCH and s["B"] * 15 <= REDUCE_BLOCKS
    s = A_ORD_CELLS
    assert STAGE < -(-cells(s["grid"]) // CELL_CHUNK) <= 2 * STAGE and -(-s["P"] // POINT_CHUNK) <= STAGE
    assert s["B"] <= LAUNCH and s["B"] * 15 <= REDUCE_BLOCKS and cells(s["grid"]) * s["B"] < 2 ** 31
    # the smooth splat: the pose stride of the forward, and pose_slices (csrc/dpr_host.h) for the pullback: 2 blocks of
    # 256 points, 1024 slices wanted, 65 poses per slice, 1010 slices; the poses around the cut lie in three of them
    # smooth sampling: the same slices for the forward and the pullback; values and ds_dvalues stay far below 2^32;
    # the last slice is partial (15 poses: the b_hi clamp) and the second block of points has idle threads
    for s in (A_SMOOTH, A_SAMPLE_SMOOTH):
        assert LAUNCH < s["B"] <= 2 * LAUNCH
        pblocks = -(-s["P"] // 256)
        wanted = min(s["B"], -(-2048 // pblocks), LAUNCH)
        per_slice = -(-s["B"] // wanted)
        assert (pblocks, wanted, per_slice, -(-s["B"] // per_slice)) == (2, 1024, 65, 1010)
        assert sorted({b // per_slice for b in around_the_cut(s["B"])}) == [0, 1008, 1009]
    s = A_SAMPLE_SMOOTH
    assert s["P"] * s["B"] < 2 ** 31 and s["P"] % 256 != 0 and 0 < s["B"] - 1009 * 65 < 65
    # Part B: the last plane / pose / cloud starts at or past element 2^32 and the one before it below; no launch
    # cut; within the entry points' own limits (check_common: grid[d] <= 32768, G <= 2^31 - 1; C, K <= 16;
    # check_sample_sizes / check_clouds_sizes: products below 2^60; ORDERED: prod (n_d + 1) <= 2^32 - 1) and
    # below 40 GB held at once
    held = {}
    for name, s, stride, big in (
            ("channels", B_CHANNELS, B_CHANNELS["C"] * cells(B_CHANNELS["grid"]), 1),
            ("jvp", B_JVP, B_JVP["K"] * cells(B_JVP["grid"]), 1),
            ("sample image", B_SAMPLE_IMAGE, cells(B_SAMPLE_IMAGE["grid"]), 2),  # image and ds_dimage
            ("sample values", B_SAMPLE_VALUES, B_SAMPLE_VALUES["P"], 1),
            ("clouds out", B_CLOUDS_OUT, cells(B_CLOUDS_OUT["grid"]), 1),
            ("clouds points", B_CLOUDS_POINTS, B_CLOUDS_POINTS["P"] * B_CLOUDS_POINTS["n_in"], 2),  # and ds_dpoints
            ("ordered", B_ORDERED, cells(B_ORDERED["grid"]), 1),
            ("smooth", B_SMOOTH, cells(B_SMOOTH["grid"]), 1),
            ("sample_smooth image", B_SAMPLE_SMOOTH_IMAGE, cells(B_SAMPLE_SMOOTH_IMAGE["grid"]), 2),  # and ds_dimage
            ("sample_smooth values", B_SAMPLE_SMOOTH_VALUES, B_SAMPLE_SMOOTH_VALUES["P"], 1)):  # then ds_dvalues
        B = s["B"]
        assert (B - 1) * stride >= 2 ** 32 > (B - 2) * stride, name
        assert B * s.get("C", s.get("K", 1)) <= LAUNCH, name
        assert all(n <= 32768 for n in s["grid"]) and cells(s["grid"]) <= 2 ** 31 - 1, name
        assert s.get("C", 1) <= 16 and s.get("K", 1) <= 16 and s["P"] < 2 ** 32, name
        assert s["P"] * B * 3 < 2 ** 60 and cells(s["grid"]) * B < 2 ** 60, name
        held[name] = big * B * stride * 4 / GB
        assert held[name] + 6 <= 40, (name, held[name])  # (+ 6 GB: comparison temporaries, the small arguments)
    assert int(np.prod([n + 1 for n in B_ORDERED["grid"]])) <= 2 ** 32 - 1
    assert (B_JVP["K"] - 1) * 2 ** 23 * 3 < 2 ** 32  # the JVP's tangent offsets: out of reach (module docstring)
    assert B_ORDERED["B"] * 15 <= REDUCE_BLOCKS and -(-B_ORDERED["P"] // POINT_CHUNK) <= STAGE
    # the smooth TILED forward takes the call: 16 x 32 x 32 tiles (3-D 16 x 8 x 8), far below its 2^31 - 1 limit
    assert int(np.prod([-(-n // e) for n, e in zip(B_SMOOTH["grid"], (16, 8, 8))])) == 16384
    # smooth sampling: the image test crosses 2^32 in b * G only (values: 257 * 100 000), the values test in b * P
    # only (images: 257 * 16^3); neither has a pose slice (one slice from 2048 blocks of points on; below, B = 257
    # poses on grid.y) nor a launch cut; the TILED planes: 16384 and 4 tiles
    assert B_SAMPLE_SMOOTH_IMAGE["B"] * B_SAMPLE_SMOOTH_IMAGE["P"] < 2 ** 31
    assert B_SAMPLE_SMOOTH_VALUES["B"] * cells(B_SAMPLE_SMOOTH_VALUES["grid"]) < 2 ** 31
    assert -(-B_SAMPLE_SMOOTH_VALUES["P"] // 256) >= 2048 > -(-B_SAMPLE_SMOOTH_IMAGE["P"] // 256)
    assert min(B_SAMPLE_SMOOTH_IMAGE["B"], -(-2048 // -(-B_SAMPLE_SMOOTH_IMAGE["P"] // 256))) <= LAUNCH
    for s, tiles in ((B_SAMPLE_SMOOTH_IMAGE, 16384), (B_SAMPLE_SMOOTH_VALUES, 4)):
        assert int(np.prod([-(-n // e) for n, e in zip(s["grid"], (16, 8, 8))])) == tiles
