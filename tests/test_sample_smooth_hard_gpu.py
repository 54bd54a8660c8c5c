"""Smooth sampling (k_sample_smooth_fwd, k_sample_smooth_bwd and the TILED pullback's planes, csrc/dpr_smooth.hip and
the driver in csrc/dpr_api_smooth.hip) in the regimes the other op families are held to: the clustered clouds with
cell-face and NaN / Inf points, a bound per value in fp32, the TILED and AUTO pullback on heavy multi-tile planes,
ds_dvalues of rejected points, the key-bit and thin-grid edges of the tiled planes, several poses per slice, the pose
order of one slice, and sample_smooth_ad on both algorithms.

Every expectation is tests/sample_smooth_reference.py (`SSR`) in fp64 on inputs rounded to fp32 once and used for both
dtypes.  The hard inputs are smooth_input("H3" | "H2_22" | "H2_32") of tests/test_smooth_hard_gpu.py (its table has
their tiles and rejected points) with an fp32-rounded image ~ N(0, 1) of shape grid + (3,) and ds_dvalues ~ N(0, 1) of
shape (P, 3) (`sample_data`).  Every pullback output of this module is a caller buffer pre-filled with 7.5: a zeroing
the library owes (ds_dpoints with several slices, ds_dimage before the tiled planes, the per-pose sums) cannot hide
on fresh memory.

The fp32 bound per value (1).  For every point p and pose b the budget, formed in fp64 from SR._terms,

    E[p, b] = sum_s |image[j0 + s, b]| ( prod_d w_d + sum_k |coord_k| |w'_k| prod_{d != k} w_d )

over the cells inside the grid: the per-cell budget of tests/test_smooth_hard_gpu.py read the other way.  The
assertion is |got - ref64| <= m E on EVERY accepted (p, b), m = M_FACTOR * rho, and got == 0 on every rejected one;
rho = max |ref32 - ref64| / E with ref32 = SSR.sample_smooth(dtype = fp32), the reference's own fp32 rounding, measured
on the CPU, never on the device (test_recorded_rho_is_the_reference_s re-measures it).  ds_dpoints (3) follows the
convention of the smooth module: max |got - ref64| <= M_FACTOR rho max |ref64|, rho of the fp32 reference per input
and batch size.

    rho, CPU reference    values       ds_dpoints B=1 / B=3
    H3                    3.857e-07    1.020e-05 / 9.351e-06
    H2_22                 2.334e-07    6.301e-06 / 6.561e-06
    H2_32                 1.268e-07    6.335e-06 / 9.173e-06

Observed on an MI355X (2026-10-19; the tests print them):
    values, fp32: max |got - ref64| / E     m           B=1 / B=3
    H3                                      1.543e-06   6.97e-08 / 3.86e-07
    H2_22                                   9.334e-07   7.57e-08 / 1.58e-07
    H2_32                                   5.071e-07   7.28e-08 / 1.94e-07
    (B = 3, H3: point 149 806 under pose 2, where the fp32 reference has its own worst value, rho to three digits;
    with the identity pose alone a fifth of it.)  Every rejected (p, b): 0.
    values against ds_dpoint_weight of the smooth pullback (2): max |difference| = 0 on all three inputs, both dtypes.

    ds_dpoints, fp32: max |got - ref64| / max |ref64| (m)    B=1                     B=3
    H3                                                       1.02e-05 (4.08e-05)     1.14e-05 (3.74e-05)
    H2_22                                                    6.20e-06 (2.52e-05)     8.87e-06 (2.62e-05)
    H2_32                                                    6.34e-06 (2.53e-05)     6.63e-06 (3.67e-05)
    the same figures on atomic, tiled and auto (one kernel) and with NaN in ds_dvalues of the rejected points (4);
    the 64 cell-face points alone: at most 4.8e-06; fp64: at most 1.3e-14 everywhere.

Derived, not measured: the tolerances of tests/test_parity_gpu.py (`tol`) wherever they are named, and every `==`.

The reference never reads ds_dvalues of a rejected point, so the expectation of (4) "with zeros there" is the
unmasked one; test_rejected_points_are_many_and_the_reference_ignores_them asserts that on the CPU.

Mutation record (scratch builds of libdpr, one MI355X run each under a time limit, the new tests of this module and
the sample_smooth tests of tests/test_index_ranges_gpu.py with -x; every mutant keeps its accesses inside its buffers:
a dropped contribution writes nothing, a wrapped offset lands earlier in the same buffer).  Each line: the mutant, the
first test and assertion that failed.
  1 k_sample_smooth_fwd: `T v = 0` hoisted out     several_poses_per_slice[2-2-float64]: values against the reference,
    of the pose loop                               7 % off (a rejected point keeps the value of the slice's first
                                                   pose).  150 tests pass before it, values_one_by_one with B = 3 among
                                                   them: its three slices hold one pose each
  2 k_sample_smooth_bwd reads ds_dvalues as dv[p]  pullback_element_by_element[H3-3-atomic-float64]: ds_dimage 112 % off
    (column 0)                                     (the B = 1 cases pass before)
  3 sample_smooth_bwd without the ds_dpoints       pullback_element_by_element[H3-3-atomic-float64]: ds_dpoints, 17 %
    memset when `accumulate` is set                off -- the 7.5 of the caller's buffer under three slices' atomics
  4 the driver's tiled loop passes `dv`, not       pullback_element_by_element[H3-3-tiled-float64]: ds_dimage, 112 % off
    `dv + b * P`                                   (atomic B = 3 passes before)
  5 pose_slices forced to two slices at            one_slice_adds_four_poses_in_index_order[2-float64]: ds_dpoints is
    P = 524 033, this entry point only             not ((p0 + p1) + p2) + p3.  164 tests pass before it, the B = 3 cases
                                                   of point_gradient_of_a_batch_at_the_slice_threshold among them
                                                   (2 + 1 poses add in the same order, as in the smooth module)
  6 `(uint32_t)(b * P)` in the forward's store     tests/test_index_ranges_gpu.py, sample_smooth_values_past_2_pow_32:
                                                   values[subsample, 256], 100 % off (this whole module passes)
  7 `(uint32_t)(b * gd.G)` on ds_dimage in         tests/test_index_ranges_gpu.py, sample_smooth_image_past_2_pow_32:
    k_sample_smooth_bwd                            atomic: ds_dimage[.., 256], 100 % off (this whole module passes)
  8 k_sample_smooth_bwd: b_hi = min(b_lo + pps,    pullback_element_by_element[H3-1-atomic-float64]: ds_dimage is 0
    B - 1), the last pose skipped                  (with B = 1 the only pose is the last one)
None survived.  Mutants of smooth_point_backward, smooth_axes and k_smooth_tile: tests/test_smooth_hard_gpu.py.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import sample_smooth_reference as SSR
from tests import smooth_reference as SR
from tests.test_families_hard_gpu import M_FACTOR, r32
from tests.test_parity_gpu import assert_close, grid_to_dev, tol
from tests.test_smooth_hard_gpu import (EDGE_CASES, EDGE_GRIDS, INPUTS, LARGE_P, N_BAD, N_FACE, TILE, coords,
                                        edge_case, frozen, large_case, pose_slice_count, smooth_input, to)

gpu = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
SEED = {"H3": 4001, "H2_22": 4002, "H2_32": 4003}
FIELDS = ("image", "points", "rotation", "translation")
KINDS = ("out", "points", "pose", "pose")
FILL = 7.5
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "values"): 3.8569e-07,
    ("H3", "points", 1): 1.0203e-05,
    ("H3", "points", 3): 9.3506e-06,
    ("H2_22", "values"): 2.3335e-07,
    ("H2_22", "points", 1): 6.3005e-06,
    ("H2_22", "points", 3): 6.5612e-06,
    ("H2_32", "values"): 1.2677e-07,
    ("H2_32", "points", 1): 6.3354e-06,
    ("H2_32", "points", 3): 9.1725e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def values_to_dev(a, tdt, dev):
    """numpy (P, B) -> device tensor with the point index fastest"""
    return to(np.asarray(a).T, tdt, dev).t()


def image_to_dev(a, tdt, dev):
    return grid_to_dev(np.array(a), dev).to(tdt)  # (a copy: the cached inputs are read-only)


def dev_args(c, s, tdt, dev, B, keep=slice(None)):
    """[image, points, rotation, translation] of the first B poses"""
    return [image_to_dev(s.image[..., :B], tdt, dev), to(c.points[keep], tdt, dev), to(c.rot[:B], tdt, dev),
            to(c.trans[:B], tdt, dev)]


def filled_outputs(grid, P, B, n_in, tdt, dev, need=FIELDS):
    """The keyword outputs of sample_smooth_pullback_, each pre-filled with 7.5"""
    n_out = len(grid)
    bufs = dict(ds_dimage=dpr_amd.empty_grid(grid, B, tdt, dev).fill_(FILL),
                ds_dpoints=torch.full((P, n_in), FILL, dtype=tdt, device=dev),
                ds_drotation=torch.full((B, n_in, n_out), FILL, dtype=tdt, device=dev).transpose(1, 2),
                ds_dtranslation=torch.full((B, n_out), FILL, dtype=tdt, device=dev))
    return {"ds_d" + f: bufs["ds_d" + f] for f in need}


def pullback(dv, args, algo, need=FIELDS):
    """sample_smooth_pullback_ into buffers pre-filled with 7.5; the wanted outputs come back by identity"""
    img, pts, rot, _trans = args
    grid, B = tuple(img.shape[:-1]), rot.shape[0]
    bufs = filled_outputs(grid, pts.shape[0], B, pts.shape[1], pts.dtype, pts.device, need)
    pb = dpr_amd.sample_smooth_pullback_(dv, *args, need=need, algo=algo, **bufs)
    for f in FIELDS:
        if f in need:
            assert getattr(pb, f).data_ptr() == bufs["ds_d" + f].data_ptr(), f"ds_d{f} is not the caller's buffer"
        else:
            assert getattr(pb, f) is None
    return pb


def check_pullback(pb, ref, npdt, what=""):
    """All four outputs finite and within the project tolerances; ds_dimage, ds_drotation and ds_dtranslation also
    pose by pose, so that a pose cannot hide in another's norm."""
    for f, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        assert bool(torch.isfinite(a).all()), f"{what}non-finite ds_d{f}"
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{what}ds_d{f}")
    B = ref[2].shape[0]
    if B <= 4:
        for b in range(B):
            assert_close(pb.image[..., b], ref[0][..., b].astype(npdt), tol(npdt, "out"), f"{what}ds_dimage[.., {b}]")
            assert_close(pb.rotation[b], ref[2][b].astype(npdt), tol(npdt, "pose"), f"{what}ds_drotation[{b}]")
            assert_close(pb.translation[b], ref[3][b].astype(npdt), tol(npdt, "pose"), f"{what}ds_dtranslation[{b}]")


# ------------------------------------------------------------------ the inputs and their references (computed once)
@functools.lru_cache(maxsize=None)
def sample_data(name):
    h = smooth_input(name)
    rng = np.random.default_rng(SEED[name])
    s = SimpleNamespace(image=r32(rng.normal(size=h.grid + (h.B,))), dv=r32(rng.normal(size=(h.P, h.B))))
    frozen(s.image, s.dv)
    return s


@functools.lru_cache(maxsize=None)
def reference_values(name, dtype=np.float64):
    """(P, 3); column b does not depend on the batch"""
    h, s = smooth_input(name), sample_data(name)
    with np.errstate(invalid="ignore"):
        v = SSR.sample_smooth(s.image, h.points, h.rot, h.trans, dtype=dtype)
    assert np.all(np.isfinite(v))
    return frozen(v)


@functools.lru_cache(maxsize=None)
def reference_pullback(name, B, dtype=np.float64):
    h, s = smooth_input(name), sample_data(name)
    with np.errstate(invalid="ignore"):
        pb = SSR.sample_smooth_pullback(s.dv[:, :B], s.image[..., :B], h.points, h.rot[:B], h.trans[:B], dtype=dtype)
    assert all(np.all(np.isfinite(x)) for x in pb)
    frozen(*pb)
    return pb


def value_budget(grid, points, rot, trans, image):
    """(E[p, b] of the module docstring, accepted[p, b]) in fp64"""
    N, P, B = len(grid), len(points), rot.shape[0]
    E, accepted = np.zeros((P, B)), np.zeros((P, B), bool)
    with np.errstate(invalid="ignore"):
        terms = list(SR._terms(grid, points, rot, trans, np.float64))
    for b, idx, j0, w, dw in terms:
        c = np.abs(coords(grid, points, rot[b], trans[b])[idx])
        e = np.zeros(len(idx))
        for st, cell, inside in SSR._cells(grid, j0, N):
            v = np.ones(len(idx))
            for d in range(N):
                v = v * w[:, d, st[d]]
            for k in range(N):
                sens = c[:, k] * np.abs(dw[:, k, st[k]])
                for d in range(N):
                    if d != k:
                        sens = sens * w[:, d, st[d]]
                v = v + sens
            a = np.zeros(len(idx))
            a[inside] = np.abs(image[..., b][tuple(cell[inside].T)])
            e += a * v
        E[idx, b] = e
        accepted[idx, b] = True
    return E, accepted


@functools.lru_cache(maxsize=None)
def budget(name):
    h, s = smooth_input(name), sample_data(name)
    return frozen(*value_budget(h.grid, h.points, h.rot, h.trans, s.image))


def measured_rho(name):
    """{key: rho} of the CPU reference, the keys of RHO."""
    E, acc = budget(name)
    v64, v32 = reference_values(name), reference_values(name, np.float32).astype(np.float64)
    assert not v32[~acc].any(), "the fp32 reference accepts a point that the fp64 reference rejects"
    assert np.all(E[acc] > 0)
    r = {(name, "values"): float((np.abs(v32 - v64)[acc] / E[acc]).max())}
    for B in (1, 3):
        p64, p32 = reference_pullback(name, B)[1], reference_pullback(name, B, np.float32)[1]
        r[(name, "points", B)] = float(np.abs(p32.astype(np.float64) - p64).max() / np.abs(p64).max())
    return r


@functools.lru_cache(maxsize=None)
def far_rejected(name):
    """(P, 3) bool: the fp64 reference rejects (p, b) by at least 1e-3 of a cell on some axis, or the point is one of
    the five with NaN / Inf coordinates."""
    h = smooth_input(name)
    n = np.asarray(h.grid, np.float64)
    far = np.zeros((h.P, h.B), bool)
    for b in range(h.B):
        c = coords(h.grid, h.points, h.rot[b], h.trans[b])
        with np.errstate(invalid="ignore"):
            far[:, b] = np.any((c < -1 - 1e-3) | (c > n + 1 + 1e-3), axis=1)
    far[-N_BAD:] = True
    return frozen(far)


# ------------------------------------------------------------------ the CPU side
@pytest.mark.parametrize("name", INPUTS)
def test_recorded_rho_is_the_reference_s(name):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 0.1 %."""
    for key, rho in measured_rho(name).items():
        print(f"rho {key}: {rho:.4e}")
        assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
        assert RHO[key] == pytest.approx(rho, rel=1e-3), f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@pytest.mark.parametrize("name", INPUTS)
def test_auto_pullback_is_tiled_for_h3_and_atomic_in_2d(name):
    """The AUTO cases of (3) do run both regimes: dpr_resolve_algo_sample_smooth from the shape alone."""
    h = smooth_input(name)
    for B in (1, 3):
        assert dpr_amd.resolve_algo_sample_smooth("pullback", h.grid, h.P, B, h.n_in) == \
            ("tiled" if name == "H3" else "atomic")
        assert dpr_amd.resolve_algo_sample_smooth("sample", h.grid, h.P, B, h.n_in) == "atomic"
    # the tail of the cloud is what the tests below take it for
    assert np.all(~np.isfinite(h.points[-N_BAD:]).all(axis=1)) and np.all(np.isfinite(h.points[:-N_BAD]))
    assert all(-(-n // e) > 1 for n, e in zip(h.grid, TILE[h.n_out])), "more than one tile on every axis"


@pytest.mark.parametrize("name", INPUTS)
def test_rejected_points_are_many_and_the_reference_ignores_them(name):
    """At least 20 points per pose that (4) poisons; all of them rejected by the reference, which gives the same
    results with NaN, with 0 and with the drawn ds_dvalues there (the smallest input: one pullback more)."""
    h, s = smooth_input(name), sample_data(name)
    far, (_E, acc) = far_rejected(name), budget(name)
    print(f"{name}: poisoned points per pose {far.sum(axis=0)}")
    assert np.all(far.sum(axis=0) >= 20) and not (far & acc).any()
    if name == "H2_22":
        with np.errstate(invalid="ignore"):
            zeroed = SSR.sample_smooth_pullback(np.where(far, 0.0, s.dv), s.image, h.points, h.rot, h.trans)
        for a, e in zip(zeroed, reference_pullback(name, 3)):
            assert np.array_equal(a, e)


# ------------------------------------------------------------------ 1 values, one by one
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_values_one_by_one(dev, name, B, npdt, tdt):
    h, s = smooth_input(name), sample_data(name)
    ref64 = reference_values(name)[:, :B]
    E, acc = (a[:, :B] for a in budget(name))
    v = dpr_amd.sample_smooth(*dev_args(h, s, tdt, dev, B))
    assert tuple(v.shape) == (h.P, B) and v.dtype == tdt and v.t().is_contiguous()
    got = v.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite values"
    assert_close(v, ref64.astype(npdt), tol(npdt, "points"), f"{name} B={B}")
    bad = ~acc & (got != 0)
    assert not bad.any(), f"{int(bad.sum())} rejected (p, b) with a value; first {tuple(np.argwhere(bad)[0])}"
    if npdt == np.float32:
        m = M_FACTOR * RHO[(name, "values")]
        d = np.abs(got - ref64)
        ratio = np.where(acc, d / np.where(acc, E, 1.0), 0.0)
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{name} B={B}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
        over = d > m * E
        assert not over.any(), f"(p, b) = {worst}: |got - ref64| = {d[worst]:.3e} > {m:.3e} * E = " \
            f"{m * E[worst]:.3e} ({int(over.sum())} values over the bound)"


# ------------------------------------------------------------------ 2 values are a pure gather
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("name", INPUTS)
def test_values_are_a_pure_gather(dev, name, npdt, tdt):
    """Column b of the batch is the single-pose call on pose b, two runs give the same bits, and for B = 1 `values`
    is the ds_dpoint_weight of the smooth pullback with ds_dout = image, out_weight = 1 and point_weight = 1 (SMOOTH
    SAMPLING of include/dpr.h: "as the ds_dpoint_weight of the smooth pullback") -- all to ==."""
    h, s = smooth_input(name), sample_data(name)
    img, pts, rot, trans = dev_args(h, s, tdt, dev, h.B)
    v = dpr_amd.sample_smooth(img, pts, rot, trans)
    assert torch.equal(v, dpr_amd.sample_smooth(img, pts, rot, trans)), "values differ between two runs"
    for b in range(h.B):
        one = dpr_amd.sample_smooth(img[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1])
        assert torch.equal(v[:, b], one[:, 0]), f"values[:, {b}] is not the column of pose {b} alone"
    ones = lambda n: torch.ones(n, dtype=tdt, device=dev)
    pb = dpr_amd.raster_pullback_smooth_(img[..., :1], pts, rot[:1], trans[:1], None, ones(1), ones(h.P))
    d = float((v[:, 0] - pb.point_weight).abs().max())
    print(f"{name} {np.dtype(npdt).name}: max |values - ds_dpoint_weight| = {d:.3e}")
    assert torch.equal(v[:, 0], pb.point_weight), f"values is not ds_dpoint_weight of the smooth pullback: {d:.3e}"


# ------------------------------------------------------------------ 3 the pullback, element by element
def check_hard_pullback(pb, name, B, npdt, what):
    """The assertions (3) and (4) share: every output finite and within its tolerance plane by plane / pose by pose,
    ds_dpoints element by element (fp32) and on the 64 cell-face rows, the five NaN / Inf rows exactly 0."""
    h = smooth_input(name)
    ref = reference_pullback(name, B)
    check_pullback(pb, ref, npdt, what)
    got, e = pb.points.cpu().numpy().astype(np.float64), ref[1]
    scale = np.abs(e).max()
    m = M_FACTOR * RHO[(name, "points", B)] if npdt == np.float32 else tol(npdt, "points")
    d = np.abs(got - e)
    faces = np.arange(h.P - N_BAD - N_FACE, h.P - N_BAD)
    print(f"{what}{np.dtype(npdt).name} ds_dpoints: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
          f"(m = {m:.3e}); face points {d[faces].max() / scale:.3e}")
    if npdt == np.float32:
        assert d.max() <= m * scale, f"{what}ds_dpoints: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} " \
            f"at point {int(np.argmax(d.max(axis=1)))}"
    row = d.max(axis=1)[faces]
    over = np.nonzero(row > m * scale)[0]
    assert len(over) == 0, f"{what}ds_dpoints of face point {int(faces[over[0]])} ({h.points[faces[over[0]]]}): off " \
        f"by {row[over[0]]:.3e} > {m:.3e} * {scale:.3e}; {len(over)} face points over the bound"
    assert not got[-N_BAD:].any(), f"{what}ds_dpoints of a NaN / Inf point is not 0"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["atomic", "tiled", "auto"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, B, algo, npdt, tdt):
    h, s = smooth_input(name), sample_data(name)
    pb = pullback(values_to_dev(s.dv[:, :B], tdt, dev), dev_args(h, s, tdt, dev, B), algo)
    check_hard_pullback(pb, name, B, npdt, f"{name} {algo} B={B} ")


# ------------------------------------------------------------------ 4 ds_dvalues of a rejected point is never used
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_ds_dvalues_of_a_rejected_point_is_never_used(dev, name, B, algo, npdt, tdt):
    """ds_dvalues[p, b] = NaN wherever the reference rejects (p, b) by at least 1e-3 of a cell and in the five
    NaN / Inf rows: nothing may read it into a result (a product with a zero weight would)."""
    h, s = smooth_input(name), sample_data(name)
    dv = np.where(far_rejected(name), np.nan, s.dv)[:, :B]
    assert np.isnan(dv).sum(axis=0).min() >= 20
    pb = pullback(values_to_dev(dv, tdt, dev), dev_args(h, s, tdt, dev, B), algo)
    check_hard_pullback(pb, name, B, npdt, f"{name} {algo} B={B}, NaN ds_dvalues: ")


# ------------------------------------------------------------------ 5 key bits and thin grids for the tiled planes
@functools.lru_cache(maxsize=None)
def edge_sample(n_in, grid):
    """edge_case's cloud and poses with an image and a ds_dvalues, and the fp64 reference."""
    c = edge_case(n_in, grid)
    rng = np.random.default_rng(6500 + n_in)
    s = SimpleNamespace(image=r32(rng.normal(size=grid + (c.B,))), dv=r32(rng.normal(size=(c.P, c.B))))
    with np.errstate(invalid="ignore"):
        s.values = SSR.sample_smooth(s.image, c.points, c.rot, c.trans)
        s.pb = SSR.sample_smooth_pullback(s.dv, s.image, c.points, c.rot, c.trans)
    assert np.all(np.isfinite(s.values)) and all(np.all(np.isfinite(x)) for x in s.pb)
    frozen(s.image, s.dv, s.values, *s.pb)
    return c, s


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid", EDGE_CASES)
def test_key_bit_and_thin_grid_edges(dev, n_in, n_out, grid, npdt, tdt):
    """1, 2, 3, 4, 7 and 8 tiles (the key bits the sort of a tiled plane sees) and axes of one or two cells."""
    assert grid in EDGE_GRIDS
    c, s = edge_sample(n_in, grid)
    args = dev_args(c, s, tdt, dev, c.B)
    v = dpr_amd.sample_smooth(*args)
    assert bool(torch.isfinite(v).all())
    assert_close(v, s.values.astype(npdt), tol(npdt, "points"), f"{grid} values")
    assert not bool((v[-6:] != 0).any()), "a never-accepted point has a value"
    dv = values_to_dev(s.dv, tdt, dev)
    assert dpr_amd.workspace_bytes_sample_smooth("pullback", grid, c.P, c.B, n_in, tdt, "tiled") > 0
    res = {}
    for algo in ("tiled", "atomic"):
        pb = res[algo] = pullback(dv, args, algo)
        check_pullback(pb, s.pb, npdt, f"{grid} {algo} ")
        assert not bool((pb.points[-6:] != 0).any()), f"{algo}: ds_dpoints of a never-accepted point is not 0"
    for b in range(c.B):
        assert_close(res["tiled"].image[..., b], res["atomic"].image[..., b].cpu().numpy(), tol(npdt, "out"),
                     f"{grid} tiled vs atomic, plane {b}")


# ------------------------------------------------------------------ 6 several poses per slice
MANY = dict(P=300, B=1031)
MANY_POSES = (0, 1, 1029, 1030)


@functools.lru_cache(maxsize=None)
def many_case(n_in, n_out):
    """300 points uniform in +-1.3 under 1031 poses on 8^N: two blocks of points (the second with 44 live threads),
    515 slices of two poses and a last slice of one."""
    from tests.test_smooth_gpu import _poses
    rng = np.random.default_rng(9000 + 10 * n_in + n_out)
    P, B, grid = MANY["P"], MANY["B"], (8,) * n_out
    rot, trans = (r32(a) for a in _poses(rng, B, n_in, n_out))
    c = SimpleNamespace(grid=grid, P=P, B=B, n_in=n_in, n_out=n_out, points=r32(rng.uniform(-1.3, 1.3, size=(P, n_in))),
                        rot=rot, trans=trans, image=r32(rng.normal(size=grid + (B,))), dv=r32(rng.normal(size=(P, B))))
    c.values = SSR.sample_smooth(c.image, c.points, c.rot, c.trans)
    c.pb = SSR.sample_smooth_pullback(c.dv, c.image, c.points, c.rot, c.trans)
    frozen(c.points, c.rot, c.trans, c.image, c.dv, c.values, *c.pb)
    return c


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_many_poses_make_slices_of_two_with_points_accepted_under_one(n_in, n_out):
    """(CPU)  pose_slices: 2 blocks, 1024 slices wanted, 2 poses per slice, 516 slices, the last of one pose (the
    b_hi clamp).  At least 400 of the 515 two-pose slices hold a point that one of their poses accepts and the other
    rejects (`live && smooth_cell` changes inside a thread's loop), at least 5 such points in rows 256 .. 299."""
    P, B = MANY["P"], MANY["B"]
    assert pose_slice_count(P, B) == (2, 516) and -(-B // 516) == 2 and B - 2 * 515 == 1
    assert P - 256 == 44
    c = many_case(n_in, n_out)
    _E, acc = value_budget(c.grid, c.points, c.rot, c.trans, c.image)
    flips = acc[:, 0:B - 1:2] ^ acc[:, 1:B:2]  # (P, 515)
    slices, rows = int(flips.any(axis=0).sum()), int(flips[256:].any(axis=1).sum())
    print(f"({n_in}, {n_out}): {slices} of 515 slices with a point accepted under one pose; {rows} such points in "
          f"rows 256 .. 299")
    assert flips.shape == (P, 515) and slices >= 400 and rows >= 5


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_several_poses_per_slice(dev, n_in, n_out, npdt, tdt):
    c = many_case(n_in, n_out)
    B = c.B
    args = dev_args(c, c, tdt, dev, B)
    img, pts, rot, trans = args
    v = dpr_amd.sample_smooth(*args)
    assert bool(torch.isfinite(v).all())
    assert_close(v, c.values.astype(npdt), tol(npdt, "points"), "values")
    for b in MANY_POSES:
        assert_close(v[:, b], c.values[:, b].astype(npdt), tol(npdt, "points"), f"values[:, {b}]")
        one = dpr_amd.sample_smooth(img[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1])
        assert torch.equal(v[:, b], one[:, 0]), f"values[:, {b}] is not the column of pose {b} alone"
    dv = values_to_dev(c.dv, tdt, dev)
    for algo in ("atomic", "tiled"):
        pb = pullback(dv, args, algo)
        check_pullback(pb, c.pb, npdt, f"{algo} ")
        for b in MANY_POSES:
            assert_close(pb.image[..., b], c.pb[0][..., b].astype(npdt), tol(npdt, "out"), f"{algo} ds_dimage[.., {b}]")
            assert_close(pb.rotation[b], c.pb[2][b].astype(npdt), tol(npdt, "pose"), f"{algo} ds_drotation[{b}]")
            assert_close(pb.translation[b], c.pb[3][b].astype(npdt), tol(npdt, "pose"), f"{algo} ds_dtranslation[{b}]")


# ------------------------------------------------------------------ 7 one slice, pose order
@functools.lru_cache(maxsize=None)
def large_sample(n):
    c = large_case(n)
    rng = np.random.default_rng(5300 + n)
    s = SimpleNamespace(image=r32(rng.normal(size=c.grid + (c.B,))), dv=r32(rng.normal(size=(len(c.points), c.B))))
    frozen(s.image, s.dv)
    return c, s


@functools.lru_cache(maxsize=None)
def large_reference(n, P):
    c, s = large_sample(n)
    return frozen(*SSR.sample_smooth_pullback(s.dv[:P, :3], s.image[..., :3], c.points[:P], c.rot[:3], c.trans[:3]))


def single_pose_points(dv, args, B):
    img, pts, rot, trans = args
    return [pullback(dv[:, b:b + 1], [img[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1]], "atomic",
                     need=("points",)).points for b in range(B)]


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("P", list(LARGE_P))
@pytest.mark.parametrize("n", [2, 3])
def test_point_gradient_of_a_batch_at_the_slice_threshold(dev, n, P, npdt, tdt):
    """P = 524 033: one slice, a thread adds its poses in index order and stores once ("summed over the poses of a
    slice in pose order", "stored with one slice" of include/dpr.h) -- the reference, the same bits run to run, and the
    bits of (p0 + p1) + p2 of the three single-pose calls, whichever other outputs are wanted.  P = 523 776: two
    slices -- the reference, and the same bits run to run (two shares onto zero commute)."""
    (c, s), B = large_sample(n), 3
    slices = pose_slice_count(P, B)[1]
    assert slices == LARGE_P[P][1]
    args = dev_args(c, s, tdt, dev, B, slice(0, P))
    dv = values_to_dev(s.dv[:P, :B], tdt, dev)
    ref = large_reference(n, P)
    pb = pullback(dv, args, "atomic", need=("points",))
    assert bool(torch.isfinite(pb.points).all())
    assert_close(pb.points, ref[1].astype(npdt), tol(npdt, "points"), f"P={P} ds_dpoints")
    again = pullback(dv, args, "atomic", need=("points",))
    assert torch.equal(pb.points, again.points), "ds_dpoints differs between two runs"
    if slices == 1:
        p = single_pose_points(dv, args, B)
        assert torch.equal(pb.points, (p[0] + p[1]) + p[2]), "ds_dpoints is not (p0 + p1) + p2 of the single-pose calls"
        full = pullback(dv, args, "atomic")
        check_pullback(full, ref, npdt, f"P={P}, all four outputs: ")
        assert torch.equal(full.points, pb.points), "ds_dpoints depends on which other outputs are wanted"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n", [2, 3])
def test_one_slice_adds_four_poses_in_index_order(dev, n, npdt, tdt):
    """B = 4 at P = 524 033: two slices would give (p0 + p1) + (p2 + p3), which differs from ((p0 + p1) + p2) + p3 on
    this input; only one thread in index order gives the latter (B = 3 cannot tell: see the smooth module)."""
    (c, s), B, P = large_sample(n), 4, max(LARGE_P)
    assert pose_slice_count(P, B) == (2048, 1) and pose_slice_count(P - 1, B) == (2047, 2)
    args = dev_args(c, s, tdt, dev, B)
    dv = values_to_dev(s.dv, tdt, dev)
    pb = pullback(dv, args, "atomic", need=("points",))
    p = single_pose_points(dv, args, B)
    serial, paired = ((p[0] + p[1]) + p[2]) + p[3], (p[0] + p[1]) + (p[2] + p[3])
    assert not torch.equal(serial, paired), "the two orders do not differ on this input"
    assert torch.equal(pb.points, serial), "ds_dpoints is not ((p0 + p1) + p2) + p3 of the single-pose calls"


# ------------------------------------------------------------------ 8 autograd
def ad_inputs(n_in, n_out, B, tdt, dev, requires=FIELDS):
    from tests.test_smooth_gpu import _poses
    rng = np.random.default_rng(8500 + 10 * n_in + n_out)
    P, grid = 50, (8,) * n_out
    rot, trans = _poses(rng, 2, n_in, n_out)
    image = image_to_dev(r32(rng.normal(size=grid + (2,)))[..., :B], tdt, dev)
    vals = [rng.uniform(-1.1, 1.1, size=(P, n_in)), rot[:B], trans[:B]]
    xs = [image] + [to(r32(v), tdt, dev) for v in vals]
    for f, x in zip(FIELDS, xs):
        x.requires_grad_(f in requires)
    return xs, values_to_dev(r32(rng.normal(size=(P, 2)))[:, :B], tdt, dev)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_autograd_equals_the_pullback(dev, n_in, n_out, B, algo, npdt, tdt):
    xs, dv = ad_inputs(n_in, n_out, B, tdt, dev)
    v = dpr_amd.sample_smooth_ad(*xs, algo=algo)
    assert v.dtype == tdt and tuple(v.shape) == (50, B)
    (v * dv).sum().backward()
    pb = pullback(dv, [x.detach() for x in xs], algo)

    def same(f, got):
        assert got is not None and got.dtype == tdt and got.shape == getattr(pb, f).shape, f
        if f == "points" and B == 1:
            assert torch.equal(got, pb.points), f"{algo}: points.grad is not ds_dpoints"
        else:
            assert_close(got, getattr(pb, f).cpu().numpy(), tol(npdt, KINDS[FIELDS.index(f)]),
                         f"{algo} B={B}: {f}.grad is not ds_d{f}")

    for f, x in zip(FIELDS, xs):
        same(f, x.grad)
    for requires in (("rotation",), ("image", "points")):
        rs, _ = ad_inputs(n_in, n_out, B, tdt, dev, requires=requires)
        (dpr_amd.sample_smooth_ad(*rs, algo=algo) * dv).sum().backward()
        for f, x in zip(FIELDS, rs):
            if f in requires:
                same(f, x.grad)
            else:
                assert x.grad is None, f"{f}.grad without requires_grad"
