"""Index ranges of the smooth splat's forward-mode derivative, in the style and shapes of
tests/test_index_ranges_gpu.py.

  (b * K + k) * G    the plane offset in k_jvp_fill, k_smooth_jvp_atomic and k_smooth_tile_jvp: 16 tangents x 17 poses
                     of 256^3 put every plane of pose 16 at or past element 2^32 (out_dot: 18 GB).  A 32-bit offset
                     lands those deposits in the planes of an earlier pose.   test_planes_past_2_pow_32
  b += gridDim.y     k_smooth_jvp_atomic strides the poses over gridDim.y = 65535, k_jvp_fill's launches are cut at
                     65535 planes: B = 65 600, K = 1.                         test_atomic_poses_across_the_launch_cut
The TILED path is left out of the second test, as the tiled smooth forward is there: it launches four kernels per
pose from the host and its per-pose loop has no cut; its plane offset is in the first.

Against tests/smooth_jvp_reference.py in fp64 on fp32 inputs, evaluated for the checked poses only; tolerance: the
norm-wise 1e-4 of tests/test_smooth_jvp_gpu.py."""
import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests import smooth_jvp_reference as JR

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
PER_POSE = ("rotation", "translation", "background", "out_weight")
PLANES = dict(K=16, B=17, grid=(256,) * 3, P=1000)
POSES = dict(K=1, B=65_600, grid=(8, 6), P=300)
LAUNCH = 65535


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def r32(a):
    return np.asarray(a, dtype=F32).astype(np.float64)


def assert_close(actual, expected, rtol, what):
    a, e = actual.detach().cpu().double().numpy(), np.asarray(expected, np.float64)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    assert np.all(np.isfinite(a)), f"{what}: non-finite values"
    err, scale = np.linalg.norm((a - e).ravel()), max(np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel()))
    assert scale > 0, what
    assert err <= rtol * scale, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


def problem(shape, n_in, seed):
    K, B, grid, P = shape["K"], shape["B"], shape["grid"], shape["P"]
    n_out = len(grid)
    rng = np.random.default_rng(seed)
    c = dict(points=r32(rng.uniform(-1.1, 1.1, size=(P, n_in))),
             rot=r32(D.random_rotations(rng, B)[:, :n_out, :n_in]), trans=r32(0.1 * rng.normal(size=(B, n_out))),
             ow=r32(rng.uniform(0.5, 2.0, size=B)), pw=r32(rng.uniform(0.5, 2.0, size=P)))
    tan = dict(points=rng.normal(size=(K, P, n_in)), rotation=rng.normal(size=(K, B, n_out, n_in)),
               translation=rng.normal(size=(K, B, n_out)), background=rng.normal(size=(K, B)),
               out_weight=rng.normal(size=(K, B)), point_weight=rng.normal(size=(K, P)))
    return c, {k: r32(v) for k, v in tan.items()}


def reference(grid, c, tan, poses, ks):
    """out_dot of the poses `poses` and tangents `ks` only: grid + (len(ks), len(poses))"""
    sub = {k + "_dot": (v[ks][:, poses] if k in PER_POSE else v[ks]) for k, v in tan.items()}
    return JR.raster_smooth_jvp(grid, c["points"], c["rot"][poses], c["trans"][poses], c["ow"][poses], c["pw"],
                                K=len(ks), **sub)


def run(grid, c, tan, K, algo, dev):
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(torch.float32)
    return dpr_amd.raster_smooth_jvp(grid, to(c["points"]), to(c["rot"]), to(c["trans"]), None, to(c["ow"]),
                                     to(c["pw"]), **{k + "_dot": to(v) for k, v in tan.items()}, tangents=K,
                                     algo=algo)


def test_planes_past_2_pow_32(dev):
    K, B, grid, P = PLANES["K"], PLANES["B"], PLANES["grid"], PLANES["P"]
    G, last = int(np.prod(grid)), B - 1
    assert last * K * G >= 2 ** 32  # every plane of the last pose lies at or past element 2^32
    assert (B * K - 1) == 271
    c, tan = problem(PLANES, 3, seed=51)
    assert np.abs(c["rot"][0] - c["rot"][last]).max() > 0.1  # poses 0 and 16 differ
    poses, ks = [0, last], [0, K - 1]
    ref = reference(grid, c, tan, poses, ks)
    assert not np.allclose(ref[..., 0], ref[..., 1])
    for algo in ("tiled", "atomic"):
        out = run(grid, c, tan, K, algo, dev)
        torch.cuda.synchronize()
        assert tuple(out.shape) == grid + (K, B)
        for j, b in enumerate(poses):
            for i, k in enumerate(ks):
                assert_close(out[..., k, b], ref[..., i, j], 1e-4, f"{algo}: plane (k, b) = ({k}, {b})")
        del out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 2)])
def test_atomic_poses_across_the_launch_cut(dev, n_in, n_out):
    K, B, grid = POSES["K"], POSES["B"], POSES["grid"]
    assert B > LAUNCH and K == 1
    c, tan = problem(POSES, n_in, seed=52 + n_in)
    poses = [0, LAUNCH - 1, LAUNCH, B - 1]
    ref = reference(grid, c, tan, poses, [0])
    out = run(grid, c, tan, K, "atomic", dev)
    torch.cuda.synchronize()
    assert tuple(out.shape) == grid + (K, B)
    for j, b in enumerate(poses):
        assert_close(out[..., 0, b], ref[..., 0, j], 1e-4, f"out_dot[.., 0, {b}]")
