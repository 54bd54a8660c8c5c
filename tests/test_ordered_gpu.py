"""DPR_ALGO_ORDERED on the GPU: the contract of include/dpr.h (SUMMATION ORDER), checked with `==`.

  1. the forward equals the serial oracle bit for bit (fp32 and fp64);
  2. ds_dpoints / ds_dpoint_weight equal the serial oracle bit for bit;
  3. the per-pose sums and ds_dbackground: same bits run to run, for a pose alone or anywhere inside a batch, and
     for the batch reversed; values within the tolerances of tests/test_parity_gpu.py (fp64 1e-10; fp32 1e-4 on the
     point gradients, 1e-3 on the per-pose sums, norm-wise);
  4. the residual pullback equals the ordered pullback of scale * (out - target), bit for bit;
  5. the workspace of exactly the queried size is respected;
  6. raster_ad(algo="ordered") gives the same gradients twice.

The clouds are those of tests/ordered_cases.py (what tests/test_ordered_host.py walks on the CPU first)."""
import functools
import re
import os

import numpy as np
import pytest
import torch

import dpr_amd
from tests import data as D
from tests import ordered_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]
PAIRS = [(2, 2), (3, 3), (3, 2), (1, 1), (2, 3), (4, 4), (3, 4)]  # (n_in, n_out)
POINT_CHUNK = int(re.search(r"#define DPR_ORDERED_POINT_CHUNK (\d+)",
                            open(os.path.join(ROOT, "include", "dpr.h")).read()).group(1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


def grid_to_dev(a, dev):
    return dpr_amd.to_grid_layout(torch.as_tensor(np.ascontiguousarray(a), device=dev))


def tol(npdt, kind):
    return 1e-10 if npdt == np.float64 else {"points": 1e-4, "pose": 1e-3}[kind]


def assert_close(actual, expected, rtol, what=""):
    a = actual.detach().cpu().numpy().astype(np.float64)
    e = np.asarray(expected, dtype=np.float64)
    assert a.shape == e.shape, f"{what}: shape {a.shape} != {e.shape}"
    err = np.linalg.norm((a - e).ravel())
    scale = max(np.linalg.norm(a.ravel()), np.linalg.norm(e.ravel()))
    assert err <= rtol * scale + 1e-300, f"{what}: |a-e|={err:.3e} > {rtol:g}*{scale:.3e}"


def assert_same_bits(actual, expected, what=""):
    """torch.equal on the values, and on the bit patterns (so a -0 / +0 or a NaN difference shows too)."""
    a = actual.detach().cpu() if isinstance(actual, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(actual))
    e = expected.detach().cpu() if isinstance(expected, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(expected))
    assert a.shape == e.shape and a.dtype == e.dtype, f"{what}: {a.shape} {a.dtype} vs {e.shape} {e.dtype}"
    if not torch.equal(a, e):
        diff = (a != e)
        k = int(diff.sum())
        i = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {k} of {a.numel()} elements differ; first at {i}: {a[i].item()!r} != {e[i].item()!r}")
    ia = a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64)
    ie = e.contiguous().view(torch.int32 if e.dtype == torch.float32 else torch.int64)
    assert torch.equal(ia, ie), f"{what}: equal values, different bit patterns"


def pose_args(d, dev, sel=None, point_weight=True):
    """(points, rotation, translation, background, out_weight, point_weight) on the device; `sel`: pose indices."""
    s = slice(None) if sel is None else sel
    return (T(d.points, dev), T(d.rotations[s], dev), T(d.translations[s], dev), T(d.backgrounds[s], dev),
            T(d.weights[s], dev), T(d.point_weights, dev) if point_weight else None)


def raster_ordered(d, dev, sel=None):
    out = dpr_amd.raster(d.grid, *pose_args(d, dev, sel), algo="ordered")
    torch.cuda.synchronize()
    return out


def pullback_ordered(d, dev, sel=None, point_weight=True, **kw):
    s = slice(None) if sel is None else sel
    g = grid_to_dev(d.ds_dout[..., s], dev)
    pb = dpr_amd.raster_pullback_(g, *pose_args(d, dev, sel, point_weight), algo="ordered", **kw)
    torch.cuda.synchronize()
    return pb


@functools.lru_cache(maxsize=None)
def case(kind, n_in, n_out, P, B, grid, npdt, seed=0):
    return C.make(kind, n_in, n_out, P, B, grid, seed=seed, dtype=npdt)


def check_forward(oracle, dev, d, npdt, what):
    ref = oracle.raster(d.grid, d.points, d.rotations, d.translations, d.backgrounds, d.weights, d.point_weights,
                        dtype=npdt)
    out = raster_ordered(d, dev)
    assert_same_bits(out, ref, what)
    return out


# ------------------------------------------------------------------ 1. forward == serial oracle
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_forward_equals_the_serial_oracle_bit_for_bit(dev, oracle, npdt, tdt, n_in, n_out):
    """B = 3, all optional arguments; 8^N grids (5000 points: ~10 contributions per cell in 3-D, so the order of the
    additions shows in the bits) at the sizes around a block, and every nasty input at P = 5000 on the awkward grid."""
    for P in (0, 1, 255, 256, 257, 5000):
        d = case("overhang", n_in, n_out, P, 3, 8, npdt, seed=P)
        out = check_forward(oracle, dev, d, npdt, f"overhang P={P}")
        assert out.dtype == tdt
    for kind in C.KINDS:
        d = case(kind, n_in, n_out, 5000, 3, C.NASTY_GRIDS[n_out], npdt, seed=11)
        check_forward(oracle, dev, d, npdt, f"{kind} on {d.grid}")
    for kind in ("centres_faces", "one_cell"):
        d = case(kind, n_in, n_out, 5000, 3, 8, npdt, seed=12)
        check_forward(oracle, dev, d, npdt, f"{kind} on 8^N")


def test_forward_more_than_one_sort_block_and_table_block(dev, oracle):
    d = case("overhang", 3, 3, 70_000, 2, (40, 40, 40), np.float32, seed=3)
    check_forward(oracle, dev, d, np.float32, "70000 points on 40^3")


@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_forward_twenty_thousand_points_in_one_cell(dev, oracle, npdt, tdt):
    d = case("one_cell", 3, 3, 20_000, 2, 8, npdt, seed=4)
    out = check_forward(oracle, dev, d, npdt, "20000 points in one cell")
    assert (out[..., 0] != float(d.backgrounds[0])).sum() <= 8  # (one reference cell: at most 2^3 cells touched)


@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2), (4, 4)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_forward_plane_is_the_same_alone_and_inside_a_batch(dev, npdt, tdt, n_in, n_out):
    d = case("overhang", n_in, n_out, 5000, 5, 8, npdt, seed=5)
    batch = raster_ordered(d, dev)
    assert_same_bits(raster_ordered(d, dev), batch, "second run")
    for b in range(d.batch):
        alone = raster_ordered(d, dev, sel=[b])
        assert_same_bits(alone[..., 0], batch[..., b], f"pose {b} alone")
    rev = raster_ordered(d, dev, sel=list(range(d.batch))[::-1])
    assert_same_bits(rev.flip(-1), batch, "reversed batch")


# ------------------------------------------------------------------ 2. per-point gradients == serial oracle
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_point_gradients_equal_the_serial_oracle_bit_for_bit(dev, oracle, npdt, tdt, n_in, n_out):
    """B = 7 at P = 1000 is where the direct kernel of DPR_ALGO_ATOMIC slices the poses and accumulates atomically."""
    for P, B in ((1000, 1), (1000, 7), (5000, 3)):
        d = case("overhang", n_in, n_out, P, B, 8, npdt, seed=20 + B)
        ref = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, d.point_weights,
                                     dtype=npdt)
        pb = pullback_ordered(d, dev)
        assert_same_bits(pb.points, ref.points, f"ds_dpoints P={P} B={B}")
        assert_same_bits(pb.point_weight, ref.point_weight, f"ds_dpoint_weight P={P} B={B}")
        # without point_weight
        ref1 = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, None, dtype=npdt)
        pb1 = pullback_ordered(d, dev, point_weight=False)
        assert_same_bits(pb1.points, ref1.points, f"ds_dpoints, default weights, P={P} B={B}")
        assert_same_bits(pb1.point_weight, ref1.point_weight, f"ds_dpoint_weight, default weights, P={P} B={B}")
        # DPR_FLAG_NO_POINT_WEIGHT_GRAD
        pb2 = pullback_ordered(d, dev, point_weight_grad=False)
        assert pb2.point_weight is None
        assert_same_bits(pb2.points, ref.points, f"ds_dpoints without the weight gradient, P={P} B={B}")


# ------------------------------------------------------------------ 3. per-pose sums and ds_dbackground
POSE_FIELDS = ("rotation", "translation", "background", "out_weight")


def check_pose_sums(dev, oracle, d, npdt):
    B = d.batch
    pb = pullback_ordered(d, dev)
    again = pullback_ordered(d, dev)
    for name, a, e in zip(pb._fields, pb, again):  # 1. two calls, all six outputs
        assert_same_bits(e, a, f"second run: {name}")
    for b in range(B):  # 2. every pose alone
        alone = pullback_ordered(d, dev, sel=[b])
        for name in POSE_FIELDS:
            assert_same_bits(getattr(alone, name)[0], getattr(pb, name)[b], f"pose {b} alone: {name}")
    rev = pullback_ordered(d, dev, sel=list(range(B))[::-1])  # 3. the batch reversed
    for name in POSE_FIELDS:
        assert_same_bits(getattr(rev, name).flip(0), getattr(pb, name), f"reversed batch: {name}")
    ref = oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights, d.point_weights,
                                 dtype=npdt)
    for name, a, e in zip(pb._fields, pb, ref):  # 4. the values
        assert_close(a, e, tol(npdt, "points" if name in ("points", "point_weight") else "pose"), name)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_pose_sums_are_reproducible_and_independent_of_the_batch(dev, oracle, npdt, tdt, n_in, n_out):
    """P = 3 chunks + 17: partials of several point chunks meet; P = 10: one partly filled sub-step; B = 7."""
    for P in (3 * POINT_CHUNK + 17, 10):
        check_pose_sums(dev, oracle, D.make(n_points=P, n_in=n_in, n_out=n_out, batch=7, grid_n=8, seed=30, dtype=npdt),
                        npdt)


def test_pose_sums_on_a_grid_of_many_cell_chunks(dev, oracle):
    d = D.make(n_points=3 * POINT_CHUNK + 17, n_in=3, n_out=3, batch=3, grid_n=64, seed=31, dtype=np.float32)
    check_pose_sums(dev, oracle, d, np.float32)


# ------------------------------------------------------------------ 4. the residual pullback
@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2), (2, 3), (4, 4)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_residual_pullback_equals_the_pullback_of_its_sensitivity(dev, npdt, tdt, n_in, n_out):
    d = case("overhang", n_in, n_out, 3 * POINT_CHUNK + 17, 3, 8 if n_out < 3 else 20 if n_out == 3 else 12, npdt, seed=40)
    args = pose_args(d, dev)
    out = dpr_amd.raster(d.grid, *args, algo="ordered")
    target = grid_to_dev(d.ds_dout, dev)
    scale = 0.7
    resid = out - target
    ds_dout = dpr_amd.to_grid_layout(torch.tensor(scale, dtype=tdt, device=dev) * resid)
    want = dpr_amd.raster_pullback_(ds_dout, *args, algo="ordered")
    # loss[b] = sum (out - target)^2 through the same chunked reduction as ds_dbackground
    want_loss = dpr_amd.raster_pullback_(dpr_amd.to_grid_layout(resid * resid), *args, algo="ordered").background
    got, loss = dpr_amd.raster_residual_pullback_(out, target, *args, scale=scale, algo="ordered")
    got2, loss2 = dpr_amd.raster_residual_pullback_(out, target, *args, scale=scale, algo="ordered")
    torch.cuda.synchronize()
    for name, a, e, a2 in zip(got._fields, got, want, got2):
        assert_same_bits(a, e, f"residual: {name}")
        assert_same_bits(a2, a, f"residual, second run: {name}")
    assert_same_bits(loss, want_loss, "loss")
    assert_same_bits(loss2, loss, "loss, second run")


# ------------------------------------------------------------------ 5. the workspace
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_workspace_of_exactly_the_queried_size_is_respected(dev, npdt, tdt):
    d = case("overhang", 3, 3, 5000, 3, 8, npdt, seed=50)
    args = pose_args(d, dev)
    g = grid_to_dev(d.ds_dout, dev)
    want_out = dpr_amd.raster(d.grid, *args, algo="ordered")
    want_pb = dpr_amd.raster_pullback_(g, *args, algo="ordered")
    pad, pattern = 4096, 0xA5
    for op in ("raster", "pullback"):
        need = dpr_amd.workspace_bytes(op, d.grid, d.n_points, d.batch, 3, tdt, "ordered")
        assert need > 0
        big = torch.full((need + 2 * pad + 256,), pattern, dtype=torch.uint8, device=dev)
        off = pad + (-(big.data_ptr() + pad)) % 256
        ws = big[off:off + need]
        assert ws.data_ptr() % 256 == 0 and ws.numel() == need
        if op == "raster":
            got = dpr_amd.raster(d.grid, *args, algo="ordered", workspace=ws)
            torch.cuda.synchronize()
            assert_same_bits(got, want_out, "out with the caller's workspace")
        else:
            got = dpr_amd.raster_pullback_(g, *args, algo="ordered", workspace=ws)
            torch.cuda.synchronize()
            for name, a, e in zip(got._fields, got, want_pb):
                assert_same_bits(a, e, f"{name} with the caller's workspace")
        assert bool((big[:off] == pattern).all()) and bool((big[off + need:] == pattern).all()), \
            f"{op}: the bytes around the workspace were written"


# ------------------------------------------------------------------ 6. autograd
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_raster_ad_ordered_gives_the_same_gradients_twice(dev, npdt, tdt):
    d = D.make(n_points=3000, n_in=3, n_out=3, batch=3, grid_n=8, seed=60, dtype=npdt)
    w = grid_to_dev(d.ds_dout, dev)

    def grads(algo):
        leaves = [t.clone().requires_grad_(True) for t in (T(d.points, dev), T(d.rotations, dev), T(d.translations, dev),
                                                           T(d.backgrounds, dev), T(d.weights, dev),
                                                           T(d.point_weights, dev))]
        out = dpr_amd.raster_ad(d.grid, *leaves, algo=algo)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), [t.grad for t in leaves]

    out1, g1 = grads("ordered")
    out2, g2 = grads("ordered")
    assert_same_bits(out2, out1, "out")
    for k, (a, b) in enumerate(zip(g1, g2)):
        assert_same_bits(b, a, f"gradient {k}")
    _, ga = grads("atomic")
    for k, (a, b) in enumerate(zip(g1, ga)):
        assert_close(a, b.cpu().numpy(), tol(npdt, "points" if k in (0, 5) else "pose"), f"gradient {k} against atomic")


def test_stage_marks_of_the_ordered_path(dev):
    """One mark around each stage: the forward walks its stages once per pose, the pullback once per call."""
    d = case("overhang", 3, 3, 5000, 3, 8, np.float32, seed=70)
    args = pose_args(d, dev)
    g = grid_to_dev(d.ds_dout, dev)
    timing = dpr_amd._pkg.timing
    t = timing.stage_times(lambda: dpr_amd.raster(d.grid, *args, algo="ordered"), "raster", "ordered", reps=2)
    assert set(t) == {"keys", "sort", "ranges", "gather", "total"} and all(v >= 0 for v in t.values())
    t = timing.stage_times(lambda: dpr_amd.raster_pullback_(g, *args, algo="ordered"), "pullback", "ordered", reps=2)
    assert set(t) == {"grid_sum", "gather", "reduce", "total"} and all(v >= 0 for v in t.values())
