"""The pullback cells of the SUMMATION ORDER table (include/dpr.h), base family and channels ATOMIC, held to `==`.

Three kinds of check, all with assert_same_bits:
  1. serial bits      the output equals the serial oracle and the device's own DPR_ALGO_ORDERED result;
  2. equivariance     f(points[perm], point_weight[perm]) == f(points, point_weight)[perm] for a fixed random perm:
                      a per-point value must not depend on the block, tile, chunk, wave or list slot of the point;
  3. repeat           four calls with the same arguments give the same bits (the weak check: never the only one
                      where 1 or 2 applies).
The inputs are the "overhang" clouds of tests/ordered_cases.py; test_inputs_tell_summation_orders_apart shows on
the CPU that their pose sums do change bits with the order, so that the `==` below can fail.

One line per cell (P = points, B = poses):

  DPR_ALGO_ATOMIC   ds_dpoints / ds_dpoint_weight, pose loop inside one thread (B == 1, or P >= 524 033):
                      serial bits: test_atomic_single_pose_point_gradients_have_the_serial_bits (B = 1),
                      test_atomic_first_unsliced_batch_has_the_serial_bits (B = 5, P = 524 033; + equivariance);
                      AUTO resolves to ATOMIC at every B = 1 shape (asserted, same bits) and to TILED at B = 5,
                      P = 524 033 (asserted: nothing to compare there)
                    ds_dpoints / ds_dpoint_weight, poses sliced (B > 1 and P <= 523 776): rounding level by contract,
                      test_atomic_sliced_batch_agrees_at_rounding_level (tol() against ORDERED, rejected points +0.0)
                    per-pose sums: rounding level by contract, compared at tol() in
                      tests/test_parity_gpu.py::test_device_equals_oracle
  DPR_ALGO_TILED    ds_dpoints / ds_dpoint_weight: test_tiled_point_gradients (equivariance + repeat: one pose, pose
                      groups, local binning, split tiles), test_tiled_pullback_on_a_kept_binning (KEEP / REUSE ==
                      the pullback that bins pose by pose)
                    per-pose sums: rounding level by contract, compared at tol() in
                      tests/test_parity_gpu.py::test_pose_groups_equal_oracle and ::test_heavy_tiles_are_split
  DPR_ALGO_CHUNKED  2-D ds_dpoints / ds_dpoint_weight, poses in one slice (B == 1, or P >= 4 190 209 and B <= 64):
                      test_chunked_2d_point_gradients_one_slice (B = 1, and B = 5 at P = 4 190 209, both for (3, 2)
                      and (2, 2): equivariance on sorted clouds, whole chunks swapped, repeat with and without
                      DPR_FLAG_COHERENT_POINTS; two slices: repeat)
                    2-D ds_dpoints / ds_dpoint_weight, three or more pose slices (small clouds, or B >= 129 at any
                      P): rounding level by contract, test_chunked_2d_sliced_batch_agrees_at_rounding_level
                    2-D per-pose sums: test_chunked_2d_pose_sums_repeat (ds_dbackground on a grid of one k_grid_sum
                      block)
                    2-D forward, one chunk, fixed-point regime (weights within a span of 2^10):
                      test_chunked_2d_forward_of_one_chunk (wider weights: rounding level, compared there)
                    3-D ds_dpoints / ds_dpoint_weight: test_chunked_3d_point_gradients (B = 1, fp32 and fp64 batches),
                      test_chunked_3d_point_gradients_through_the_inside_sort
                    3-D per-pose sums: test_chunked_3d_point_gradients (repeat: B = 1 all four; fp64 batches
                      ds_drotation / ds_dtranslation / ds_dout_weight); the fp32 batch kernel and the batch kernels'
                      ds_dbackground: rounding level by contract, compared at tol() in
                      tests/test_owner_gpu.py::test_odd_grid_shapes
  channels ATOMIC   ds_dpoints / ds_dpoint_weight, pose loop inside one thread: test_channels_atomic_point_gradients
                      (equivariance + repeat at B = 1 and at B = 5, P = 524 033)
                    ds_dpoints / ds_dpoint_weight, poses sliced: rounding level by contract,
                      test_channels_atomic_sliced_batch_agrees_at_rounding_level
                    per-pose sums: rounding level by contract, compared at tol() in
                      tests/test_channels_gpu.py::test_pullback_decomposes_over_channels
"""
import copy
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import ordered_cases as C
from tests.test_ordered_gpu import (DTYPES, PAIRS, T, assert_close, assert_same_bits, case, dev,  # noqa: F401 (dev: fixture)
                                    grid_to_dev, tol)
from tests.test_parity_gpu import tol as parity_tol  # (has the forward's tolerance, "out")

gpu = pytest.mark.gpu

POINT_FIELDS = ("points", "point_weight")
POSE_FIELDS = ("rotation", "translation", "background", "out_weight")
SMALL_SIZES = (1, 255, 256, 257, 5000)
UNSLICED_P = 524_033  # 2048 blocks of 256 points: the first size at which pose_slices() keeps a batch in one slice
TILED_DIMS = [(3, 3), (3, 2), (2, 2)]


# ------------------------------------------------------------------ inputs (shared with the CPU test below)
def a2_case(n_in, n_out, npdt):
    return case("overhang", n_in, n_out, UNSLICED_P, 5, 8, npdt, seed=7)


FAR_POINT = 3  # index of a point that every pose rejects


@functools.lru_cache(maxsize=None)
def a4_case(n_in, n_out, npdt):
    """B = 7 at P = 1000: seven pose slices.  Point 3 is moved far off the grid."""
    d = copy.copy(case("overhang", n_in, n_out, 1000, 7, 8, npdt, seed=27))
    d.points = d.points.copy()
    d.points[FAR_POINT] = 50.0
    return d


# path -> (n_in, n_out) -> (grid, P, B); the shapes of the existing tests that reach the path
TILED_SHAPES = {
    # tests/test_parity_gpu.py::test_pose_groups_equal_oracle (its grids and batches), one pose
    "single": {(3, 3): (40, 30_000, 1), (3, 2): (96, 30_000, 1), (2, 2): (64, 30_000, 1)},
    # tests/test_parity_gpu.py::test_pose_groups_equal_oracle: groups of 16 / 4 / 2 / 1 poses (any P forms them)
    "groups": {(3, 3): (40, 30_000, 19), (3, 2): (96, 30_000, 21), (2, 2): (64, 30_000, 7)},
    # tests/test_configs_gpu.py::test_local_binning_of_coherent_points (its grids and P; five poses instead of two,
    # so that the order of the pose sum can show)
    "local": {(3, 3): (70, 150_000, 5), (3, 2): (150, 150_000, 5), (2, 2): (100, 150_000, 5)},
    # tests/test_parity_gpu.py::test_heavy_tiles_are_split (its grids and P; five poses instead of two)
    "heavy": {(3, 3): (70, 40_000, 5), (3, 2): (90, 40_000, 5), (2, 2): (64, 40_000, 5)},
    # tests/test_parity_gpu.py::test_batched_pullback_reusing_forward_binning (its grids and P; seven poses: the
    # pullback that bins for itself forms groups of 4 + 2 + 1)
    "reuse": {(3, 3): ((40, 40, 40), 30_000, 7), (3, 2): ((90, 70), 30_000, 7), (2, 2): ((90, 70), 30_000, 7)},
}
TILED_KW = {"single": {}, "groups": {}, "heavy": {}, "reuse": {},
            "local": dict(coherent_points=True, max_pose_group=1)}  # (one pose per group selects the local bins)


@functools.lru_cache(maxsize=None)
def tiled_case(path, n_in, n_out, npdt):
    grid, P, B = TILED_SHAPES[path][(n_in, n_out)]
    d = C.make("overhang", n_in, n_out, P, B, grid, seed=41 + len(path), dtype=npdt)
    if path == "groups":  # a clustered cloud: some (pose, tile) bins split
        d.points[: 2 * P // 3] *= npdt(0.3)
        d.points[::11] *= npdt(5.0)
    elif path == "local":
        d.points[::13] *= npdt(3.0)   # some far outside
        d.points[1::5] *= npdt(0.05)  # a tight cluster: heavy tiles are split into parts
    elif path == "heavy":
        d.points = (d.points * npdt(0.12)).astype(npdt)  # a few tiles hold everything
        d.points[::50] *= npdt(8.0)                      # plus some stragglers elsewhere
    elif path == "reuse":
        d.points[::9] *= npdt(3.0)
    return d


SENSITIVITY_INPUTS = ([("A2", a2_case, dims) for dims in [(3, 3), (3, 2)]]
                      + [("A4", a4_case, dims) for dims in PAIRS]
                      + [(path, functools.partial(tiled_case, path), dims)
                         for path in ("groups", "local", "heavy", "reuse") for dims in TILED_DIMS])


@pytest.mark.parametrize("name,make,dims", SENSITIVITY_INPUTS, ids=[f"{n}-{d[0]}{d[1]}" for n, _, d in SENSITIVITY_INPUTS])
def test_inputs_tell_summation_orders_apart(oracle, name, make, dims):
    """CPU only, by the oracle alone: the per-pose point gradients of the batch inputs below (fp32), one pose per
    oracle call, added in numpy in fp32 once in index order and once reversed.  At least a tenth of the elements
    of ds_dpoints must differ in bits -- on an input where every order gives the same bits, every `==` of this
    module would hold whatever the kernels do.  Measured shares of differing elements:
      A2 (B = 5, P = 524 033)   (3,3) 0.280  (3,2) 0.318
      A4 (B = 7, P = 1000)      (2,2) 0.446  (3,3) 0.376  (3,2) 0.429  (1,1) 0.527  (2,3) 0.464  (4,4) 0.320  (3,4) 0.409
      tiled, pose groups        (3,3) 0.606  (3,2) 0.681  (2,2) 0.495
      tiled, local binning      (3,3) 0.282  (3,2) 0.323  (2,2) 0.340
      tiled, split tiles        (3,3) 0.494  (3,2) 0.489  (2,2) 0.503
      tiled, kept binning       (3,3) 0.287  (3,2) 0.351  (2,2) 0.353"""
    d = make(*dims, np.float32)
    per_pose = [oracle.raster_pullback(d.ds_dout[..., b:b + 1], d.points, d.rotations[b:b + 1], d.translations[b:b + 1],
                                       d.weights[b:b + 1], d.point_weights, dtype=np.float32).points
                for b in range(d.batch)]
    fwd = np.zeros_like(per_pose[0])
    rev = np.zeros_like(per_pose[0])
    for k in range(d.batch):
        fwd = fwd + per_pose[k]
        rev = rev + per_pose[d.batch - 1 - k]
    assert fwd.dtype == np.float32 and rev.dtype == np.float32
    share = float((fwd.view(np.int32) != rev.view(np.int32)).mean())
    print(f"{name} {dims}: {share:.3f} of the ds_dpoints elements change bits with the pose order")
    assert share >= 0.1, f"{name} {dims}: only {share:.3f} of the elements depend on the order"


# ------------------------------------------------------------------ helpers
def random_perm(n_points, dev, seed=1):
    return torch.as_tensor(np.random.default_rng(seed).permutation(n_points), device=dev)


class Problem:
    """The tensors of a case on the device, and its pullbacks."""

    def __init__(self, d, dev):
        self.d, self.dev = d, dev
        self.g = grid_to_dev(d.ds_dout, dev)
        self.pts, self.pw = T(d.points, dev), T(d.point_weights, dev)
        self.pose = (T(d.rotations, dev), T(d.translations, dev), T(d.backgrounds, dev), T(d.weights, dev))

    def args(self, perm=None, point_weight=True):
        pts = self.pts if perm is None else self.pts[perm].contiguous()
        pw = None if not point_weight else (self.pw if perm is None else self.pw[perm].contiguous())
        return (pts, *self.pose, pw)

    def pullback(self, algo, perm=None, point_weight=True, **kw):
        pb = dpr_amd.raster_pullback_(self.g, *self.args(perm, point_weight), algo=algo, **kw)
        torch.cuda.synchronize()
        return pb

    def perm(self, seed=1):
        return random_perm(self.pts.shape[0], self.dev, seed)


def check_point_bits(got, want, what):
    assert_same_bits(got.points, want.points, f"{what}: ds_dpoints")
    if got.point_weight is None or want.point_weight is None:
        assert got.point_weight is None and want.point_weight is None, f"{what}: ds_dpoint_weight"
    else:
        assert_same_bits(got.point_weight, want.point_weight, f"{what}: ds_dpoint_weight")


def check_equivariance(run, perm, what):
    """Check 2.  `run(perm)` is the pullback of the cloud permuted by `perm` (None: as it is)."""
    base = run(None)
    moved = run(perm)
    assert_same_bits(moved.points, base.points[perm], f"{what}: ds_dpoints of the permuted cloud")
    if base.point_weight is not None:
        assert_same_bits(moved.point_weight, base.point_weight[perm], f"{what}: ds_dpoint_weight of the permuted cloud")
    return base


def check_repeat(run, fields, what, first=None):
    """Check 3: four calls, the same bits in `fields`."""
    first = run() if first is None else first
    for k in range(3):
        again = run()
        for name in fields:
            assert_same_bits(getattr(again, name), getattr(first, name), f"{what}: {name}, call {k + 2}")


def check_rounding_level(got, want, npdt, what):
    for name, a, e in zip(got._fields, got, want):
        assert_close(a, e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else e,
                     tol(npdt, "points" if name in POINT_FIELDS else "pose"), f"{what}: {name}")


def check_rejected_points_are_plus_zero(got, ref, tdt, what):
    """Points that every pose rejects (the oracle's gradients are all zero): +0.0 exactly, never -0.0 or garbage."""
    rejected = np.flatnonzero((ref.points == 0).all(axis=1) & (ref.point_weight == 0))
    assert FAR_POINT in rejected, f"{what}: point {FAR_POINT} was meant to be off the grid in every pose"
    idx = torch.as_tensor(rejected, device=got.points.device)
    assert_same_bits(got.points[idx], torch.zeros((len(rejected), got.points.shape[1]), dtype=tdt), f"{what}: ds_dpoints")
    if got.point_weight.ndim == 1:
        assert_same_bits(got.point_weight[idx], torch.zeros(len(rejected), dtype=tdt), f"{what}: ds_dpoint_weight")


def oracle_pullback(oracle, d, npdt, point_weight=True):
    return oracle.raster_pullback(d.ds_dout, d.points, d.rotations, d.translations, d.weights,
                                  d.point_weights if point_weight else None, dtype=npdt)


def auto_algo(d):
    return dpr_amd.resolve_algo("pullback", d.grid, d.n_points, d.batch, d.n_in)


# ------------------------------------------------------------------ A. DPR_ALGO_ATOMIC
@gpu
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_atomic_single_pose_point_gradients_have_the_serial_bits(dev, oracle, npdt, tdt, n_in, n_out):
    """A1 and A3.  B = 1: k_bwd_gather is k_ord_bwd operation for operation, so ds_dpoints / ds_dpoint_weight are
    the oracle's bits and DPR_ALGO_ORDERED's -- with point weights, with the default ones and without the weight
    gradient; sizes around a block of 256 points.  AUTO resolves to ATOMIC on every one of these shapes (asserted)
    and gives the same bits."""
    for P in SMALL_SIZES:
        d = case("overhang", n_in, n_out, P, 1, 8, npdt, seed=100 + P)
        p = Problem(d, dev)
        for pw, kw in ((True, {}), (False, {}), (True, dict(point_weight_grad=False))):
            what = f"P={P} point_weight={pw} {kw}"
            ref = oracle_pullback(oracle, d, npdt, pw)
            got = p.pullback("atomic", point_weight=pw, **kw)
            assert got.points.dtype == tdt
            assert_same_bits(got.points, ref.points, f"{what}: ds_dpoints against the oracle")
            if kw:
                assert got.point_weight is None
            else:
                assert_same_bits(got.point_weight, ref.point_weight, f"{what}: ds_dpoint_weight against the oracle")
            check_point_bits(got, p.pullback("ordered", point_weight=pw, **kw), f"{what}, against ORDERED")
            assert auto_algo(d) == "atomic"  # (every pair, every size here)
            check_point_bits(p.pullback("auto", point_weight=pw, **kw), got, f"{what}, AUTO")


@gpu
@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2)])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_atomic_first_unsliced_batch_has_the_serial_bits(dev, oracle, npdt, tdt, n_in, n_out):
    """A2.  B = 5 at P = 524 033, the first size of 2048 blocks: pose_slices() keeps the five poses inside the
    thread.  (A3: AUTO resolves to TILED at this shape, so there is no ATOMIC result of AUTO to compare.)  Serial bits against DPR_ALGO_ORDERED and against the oracle (its serial run of the 2.6 M
    point-poses takes well under a second), then equivariance."""
    d = a2_case(n_in, n_out, npdt)
    p = Problem(d, dev)
    got = check_equivariance(lambda perm: p.pullback("atomic", perm), p.perm(), "atomic")
    check_point_bits(got, p.pullback("ordered"), "against ORDERED")
    ref = oracle_pullback(oracle, d, npdt)
    assert_same_bits(got.points, ref.points, "ds_dpoints against the oracle")
    assert_same_bits(got.point_weight, ref.point_weight, "ds_dpoint_weight against the oracle")
    # A3: AUTO leaves ATOMIC for TILED at this shape, so it has no ATOMIC result to compare (test_tiled_* hold
    # what it runs instead); should the rule change, this assert says that the comparison is due here
    assert auto_algo(d) == "tiled", "AUTO at B = 5, P = 524 033 on 8^N"


@gpu
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_atomic_sliced_batch_agrees_at_rounding_level(dev, oracle, npdt, tdt, n_in, n_out):
    """A4.  B = 7 at P = 1000: seven pose slices whose shares meet in float atomics on zeroed buffers -- no bit
    claim (include/dpr.h).  All six outputs within tol() of DPR_ALGO_ORDERED; a point that every pose rejects
    keeps the +0.0 of the memset."""
    d = a4_case(n_in, n_out, npdt)
    p = Problem(d, dev)
    got = p.pullback("atomic")
    check_rounding_level(got, p.pullback("ordered"), npdt, "against ORDERED")
    check_rejected_points_are_plus_zero(got, oracle_pullback(oracle, d, npdt), tdt, "sliced")


# ------------------------------------------------------------------ B. DPR_ALGO_TILED
@gpu
@pytest.mark.parametrize("path", ["single", "groups", "local", "heavy"])
@pytest.mark.parametrize("n_in,n_out", TILED_DIMS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_tiled_point_gradients(dev, npdt, tdt, n_in, n_out, path):
    """One gradient record per (point, pose), added per point in a fixed order: equivariance and repeat for one
    pose, a batch binned in pose groups, DPR_FLAG_COHERENT_POINTS local binning and a cloud that splits heavy
    tiles (TILED_SHAPES names the test each shape comes from)."""
    p = Problem(tiled_case(path, n_in, n_out, npdt), dev)
    kw = TILED_KW[path]
    base = check_equivariance(lambda perm: p.pullback("tiled", perm, **kw), p.perm(), path)
    check_repeat(lambda: p.pullback("tiled", **kw), POINT_FIELDS, path, first=base)


@gpu
@pytest.mark.parametrize("n_in,n_out", TILED_DIMS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_tiled_pullback_on_a_kept_binning(dev, npdt, tdt, n_in, n_out):
    """A KEEP_BINNING forward followed by a REUSE_BINNING pullback, seven poses: ds_dpoints / ds_dpoint_weight are
    the bits of the pullback that bins for itself pose by pose (DPR_FLAG_MAX_POSE_GROUP(1)): both add a point's
    seven records in index order.  The default self-binning pullback forms groups of 4 + 2 + 1 poses and adds
    (g0 + g1 + g2 + g3) + (g4 + g5) + g6: another association, rounding level (include/dpr.h).  Equivariance of
    the kept pair as well.  The per-pose sums are rounding level within a tile and are not compared."""
    d = tiled_case("reuse", n_in, n_out, npdt)
    p = Problem(d, dev)
    need = max(dpr_amd.workspace_bytes(op, d.grid, d.n_points, d.batch, n_in, tdt, "tiled", sharing=True)
               for op in ("raster", "pullback"))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = dpr_amd.empty_grid(d.grid, d.batch, tdt, dev)

    def kept(perm):
        args = p.args(perm)
        dpr_amd.raster_(out, *args, algo="tiled", workspace=ws, keep_binning=True)
        pb = dpr_amd.raster_pullback_(p.g, *args, algo="tiled", workspace=ws, reuse_binning=True)
        torch.cuda.synchronize()
        return pb

    got = check_equivariance(kept, p.perm(), "kept binning")
    assert not bool(torch.isnan(got.points).any())
    check_point_bits(got, p.pullback("tiled", max_pose_group=1), "against the pullback that bins pose by pose")
    grouped = p.pullback("tiled")
    for name in POINT_FIELDS:
        assert_close(getattr(got, name), getattr(grouped, name).cpu().numpy(), tol(npdt, "points"),
                     f"against the pullback that bins pose groups: {name}")


# ------------------------------------------------------------------ C. DPR_ALGO_CHUNKED, 2-D grids
CHUNK = 4096  # points per chunk of the 2-D chunk-owner kernels
CHUNKED_2D = [(3, 2), (2, 2)]


def sorted_problem(d, dev):
    """`d` with the cloud in dpr_amd.sort_points order (what DPR_FLAG_COHERENT_POINTS is for)."""
    p = Problem(d, dev)
    p.pts, _, p.pw = dpr_amd.sort_points(p.pts, p.pw)
    return p


def swap_first_two_chunks(P, dev):
    idx = torch.arange(P, device=dev)
    idx[:CHUNK], idx[CHUNK:2 * CHUNK] = torch.arange(CHUNK, 2 * CHUNK, device=dev), torch.arange(CHUNK, device=dev)
    return idx


def check_chunked_2d_one_slice(dev, d):
    p = sorted_problem(d, dev)
    coherent = lambda perm=None: p.pullback("chunked", perm, coherent_points=True)
    base = check_equivariance(coherent, p.perm(), "sorted cloud, permuted")
    check_equivariance(coherent, swap_first_two_chunks(d.n_points, dev), "sorted cloud, two whole chunks swapped")
    check_repeat(coherent, POINT_FIELDS, "with the flag", first=base)
    unsorted = Problem(d, dev)
    check_repeat(lambda: unsorted.pullback("chunked"), POINT_FIELDS, "without the flag (sorted inside the call)")


@gpu
@pytest.mark.parametrize("n_in,n_out", CHUNKED_2D)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_2d_point_gradients_one_slice(dev, npdt, tdt, n_in, n_out):
    """The poses of a chunk run inside one block (co_plan: B == 1, or at least 1024 chunks and B <= 64, the most
    a block takes): a point's gradients stay in registers across the poses -- equivariance on a sorted cloud under a random permutation and with two
    whole 4096-point chunks swapped, repeat with and without DPR_FLAG_COHERENT_POINTS.  P = 3 chunks + 17 for one
    pose; B = 5 at the first size of 1024 chunks, P = 4 190 209.  Two slices (B = 2) add two shares to a zeroed
    buffer, which commutes: the same bits run to run."""
    check_chunked_2d_one_slice(dev, C.make("overhang", n_in, n_out, 3 * CHUNK + 17, 1, 64, seed=51, dtype=npdt))
    check_chunked_2d_one_slice(dev, C.make("overhang", n_in, n_out, 1023 * CHUNK + 1, 5, 64, seed=52, dtype=npdt))
    two = sorted_problem(C.make("overhang", n_in, n_out, 3 * CHUNK + 17, 2, 64, seed=53, dtype=npdt), dev)
    check_repeat(lambda: two.pullback("chunked", coherent_points=True), POINT_FIELDS, "two pose slices")


@gpu
@pytest.mark.parametrize("n_in,n_out", CHUNKED_2D)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_2d_sliced_batch_agrees_at_rounding_level(dev, oracle, npdt, tdt, n_in, n_out):
    """B = 5 at P = 3 chunks + 17: co_plan cuts the poses into five slices on grid.y whose shares of ds_dpoints /
    ds_dpoint_weight meet in float atomics on zeroed buffers, like the sliced DPR_ALGO_ATOMIC kernel -- no bit
    claim (include/dpr.h).  Within tol() of DPR_ALGO_ORDERED, with and without the flag."""
    d = C.make("overhang", n_in, n_out, 3 * CHUNK + 17, 5, 64, seed=54, dtype=npdt)
    p = Problem(d, dev)
    want = p.pullback("ordered")
    check_rounding_level(p.pullback("chunked"), want, npdt, "without the flag")
    check_rounding_level(p.pullback("chunked", coherent_points=True), want, npdt, "with the flag")


@gpu
@pytest.mark.parametrize("n_in,n_out", CHUNKED_2D)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_2d_pose_sums_repeat(dev, npdt, tdt, n_in, n_out):
    """DPR_FLAG_COHERENT_POINTS, B = 5, P = 3 chunks + 17 (chunk partials meet): a (chunk, pose) is summed by one
    block as a fixed tree, the partials per (chunk, pose) in f64 in a fixed order -- ds_drotation, ds_dtranslation
    and ds_dout_weight repeat bit for bit, however the poses are sliced.  ds_dbackground is k_grid_sum's: one
    block, so a fixed order, on this grid of 64^2 = 4096 cells."""
    p = sorted_problem(C.make("overhang", n_in, n_out, 3 * CHUNK + 17, 5, 64, seed=55, dtype=npdt), dev)
    check_repeat(lambda: p.pullback("chunked", coherent_points=True), POSE_FIELDS, "per-pose sums")


@gpu
@pytest.mark.parametrize("n_in,n_out", CHUNKED_2D)
def test_chunked_2d_forward_of_one_chunk(dev, n_in, n_out):
    """fp32, DPR_FLAG_COHERENT_POINTS, P = 4000 (one chunk), B = 5: exact fixed-point sums per chunk and one flush
    per cell onto the background -- `out` repeats bit for bit and does not depend on the order of the points.
    That holds in the fixed-point regime only (include/dpr.h, note 3): non-zero |point_weight| of the chunk within
    a span of 2^10.  So `==` with the default weights and with the overhang weights clamped to [2^-4, 2^4] (both
    signs, a span of 2^8); the overhang weights as they are span more than 2^12, which switches the chunk to f64
    LDS atomics: rounding level, compared at the forward's tolerance."""
    d = C.make("overhang", n_in, n_out, 4000, 5, 64, seed=56, dtype=np.float32)
    p = sorted_problem(d, dev)
    perm = p.perm()
    narrow = torch.sign(p.pw) * p.pw.abs().clamp(2.0 ** -4, 2.0 ** 4)
    for what, pw in (("default weights", None), ("weights within a span of 2^8", narrow)):
        run = lambda q=None: dpr_amd.raster(d.grid, p.pts if q is None else p.pts[q].contiguous(), *p.pose,
                                            pw if pw is None or q is None else pw[q].contiguous(),
                                            algo="chunked", coherent_points=True)
        out = run()
        for k in range(3):
            assert_same_bits(run(), out, f"{what}: out, call {k + 2}")
        assert_same_bits(run(perm), out, f"{what}: out of the permuted cloud")
    wide = dpr_amd.raster(d.grid, *p.args(), algo="chunked", coherent_points=True)
    assert_close(wide, dpr_amd.raster(d.grid, *p.args(), algo="ordered").cpu().numpy(), parity_tol(np.float32, "out"),
                 "overhang weights: out")


# ------------------------------------------------------------------ D. DPR_ALGO_CHUNKED, 3-D grids
@gpu
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_3d_point_gradients(dev, npdt, tdt, batch):
    """One thread per point, the poses added in index order (registers across a launch of up to 64 poses):
    equivariance and repeat for one pose and for a batch of five in fp32 and fp64; P = 20 000 on 40^3, which
    tests/test_owner_gpu.py::test_odd_grid_shapes shows the path accepts.  Per-pose sums, repeat only where the
    order is fixed: one pose (all four), fp64 batches (ds_drotation, ds_dtranslation, ds_dout_weight: parked per
    thread and summed by one wave per value; their ds_dbackground and every sum of the fp32 batch kernel meet in
    f64 LDS atomics in arrival order)."""
    p = Problem(C.make("overhang", 3, 3, 20_000, batch, 40, seed=61, dtype=npdt), dev)
    base = check_equivariance(lambda perm: p.pullback("chunked", perm), p.perm(), f"B={batch}")
    fields = POINT_FIELDS
    if batch == 1:
        fields += POSE_FIELDS
    elif npdt == np.float64:
        fields += ("rotation", "translation", "out_weight")
    check_repeat(lambda: p.pullback("chunked"), fields, f"B={batch}", first=base)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_chunked_3d_point_gradients_through_the_inside_sort(dev, npdt, tdt):
    """B >= 8, P >= 200 000 and no flag: the cloud is Hilbert-sorted inside the call and the gradients come back
    through the inverse permutation -- still equivariant and repeatable.  The smallest shape of
    tests/test_owner_gpu.py::test_unsorted_batch_is_sorted_inside_the_pullback."""
    d = C.make("overhang", 3, 3, 210_000, 9, (40, 33, 29), seed=62, dtype=npdt)
    assert dpr_amd.workspace_bytes("pullback", d.grid, d.n_points, d.batch, 3, tdt, "chunked") \
        > 2 * d.n_points * 3 * np.dtype(npdt).itemsize  # (sorted copy + sorted gradients: the sorting variant)
    p = Problem(d, dev)
    base = check_equivariance(lambda perm: p.pullback("chunked", perm), p.perm(), "inside sort")
    check_repeat(lambda: p.pullback("chunked"), POINT_FIELDS, "inside sort", first=base)


# ------------------------------------------------------------------ E. channels, DPR_ALGO_ATOMIC
N_CHANNELS = 3


class ChannelProblem:
    """`d` with three channels of weights (both signs, over 2^12) and a sensitivity per channel."""

    def __init__(self, d, dev, tdt, seed):
        rng = np.random.default_rng(seed)
        P, B = d.n_points, d.batch
        self.d, self.dev = d, dev
        dt = d.points.dtype
        self.pw_host = (rng.normal(size=(P, N_CHANNELS)) * np.exp2(rng.uniform(-6, 6, size=(P, N_CHANNELS)))).astype(dt)
        self.g_host = rng.normal(size=tuple(d.grid) + (N_CHANNELS, B)).astype(dt)
        self.g = dpr_amd.empty_channel_grid(d.grid, N_CHANNELS, B, tdt, dev)
        self.g.copy_(torch.as_tensor(self.g_host, device=dev))
        self.pts, self.pw = T(d.points, dev), T(self.pw_host, dev)
        self.pose = (T(d.rotations, dev), T(d.translations, dev), T(d.weights, dev))

    def pullback(self, perm=None):
        pts = self.pts if perm is None else self.pts[perm].contiguous()
        pw = self.pw if perm is None else self.pw[perm].contiguous()
        pb = dpr_amd.raster_pullback_channels_(self.g, pts, self.pose[0], self.pose[1], pw, None, self.pose[2],
                                               algo="atomic")
        torch.cuda.synchronize()
        return pb

    perm = Problem.perm


@gpu
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_channels_atomic_point_gradients(dev, npdt, tdt, n_in, n_out):
    """C = 3, the pose loop inside one thread: B = 1 at the sizes around a block, and (3-D points only) B = 5 at
    P = 524 033.  The table does not imply the bits of a single-channel call on folded weights (the channels are
    folded per gather), so equivariance and repeat."""
    cases = [case("overhang", n_in, n_out, P, 1, 8, npdt, seed=100 + P) for P in SMALL_SIZES]
    if (n_in, n_out) in ((3, 3), (3, 2)):
        cases.append(a2_case(n_in, n_out, npdt))
    for d in cases:
        p = ChannelProblem(d, dev, tdt, seed=71)
        what = f"P={d.n_points} B={d.batch}"
        base = check_equivariance(p.pullback, p.perm(), what)
        check_repeat(p.pullback, POINT_FIELDS, what, first=base)


@gpu
@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt,tdt", DTYPES)
def test_channels_atomic_sliced_batch_agrees_at_rounding_level(dev, npdt, tdt, n_in, n_out):
    """C = 3, B = 7 at P = 1000: seven pose slices, float atomics on zeroed buffers, no bit claim.  Within tol() of
    the channel-wise DPR_ALGO_ORDERED pullbacks (ds_dpoints and the pose gradients summed over the channels in
    f64 on the host); a point that every pose rejects keeps +0.0."""
    d = a4_case(n_in, n_out, npdt)
    p = ChannelProblem(d, dev, tdt, seed=72)
    got = p.pullback()
    single = Problem(d, dev)
    sums = {name: 0.0 for name in ("points", "rotation", "translation", "out_weight")}
    for c in range(N_CHANNELS):
        single.g = grid_to_dev(p.g_host[..., c, :], dev)
        single.pw = p.pw[:, c].contiguous()
        pb = single.pullback("ordered")
        for name in sums:
            sums[name] = sums[name] + getattr(pb, name).double().cpu().numpy()
        assert_close(got.point_weight[:, c], pb.point_weight.cpu().numpy(), tol(npdt, "points"), f"ds_dpoint_weight[:, {c}]")
        assert_close(got.background[:, c], pb.background.cpu().numpy(), tol(npdt, "pose"), f"ds_dbackground[:, {c}]")
        if c == 0:
            rejected = torch.nonzero((pb.points == 0).all(dim=1) & (pb.point_weight == 0)).ravel()
    for name, e in sums.items():
        assert_close(getattr(got, name), e, tol(npdt, "points" if name == "points" else "pose"), name)
    assert FAR_POINT in rejected.tolist()
    assert_same_bits(got.points[rejected], torch.zeros((len(rejected), n_in), dtype=tdt), "ds_dpoints of rejected points")
    assert_same_bits(got.point_weight[rejected], torch.zeros((len(rejected), N_CHANNELS), dtype=tdt),
                     "ds_dpoint_weight of rejected points")
