"""Smooth sampling at the points of rigid bodies (k_sample_smooth_bodies_fwd, k_sample_smooth_bodies_bwd and
k_sample_smooth_bodies_tile of csrc/dpr_sample_smooth_bodies.hip) on the hard body input of
tests/test_smooth_bodies_hard_gpu.py (`bodies_input`: B = 3 images, K = 3 bodies, sorted and shuffled labels, dropped
points inside the heavy runs; its docstring has the regime table), with the image and the ds_dvalues of `sample_data`
of tests/test_sample_smooth_hard_gpu.py.

Every expectation is tests/sample_smooth_bodies_reference.py (`SBR`) in fp64 on inputs rounded to fp32 once and used
for both dtypes.  Every pullback output is a caller buffer pre-filled with 7.5 (sorted) or NaN (shuffled).

Values, fp32: |got - ref64| <= M_FACTOR rho E[p, b] on EVERY accepted (p, b), E the `value_budget` of
tests/test_sample_smooth_hard_gpu.py evaluated per body subset under the body's poses; exactly 0 on every rejected or
dropped (p, b).  ds_dpoints: max |got - ref64| <= M_FACTOR rho max |ref64| (all rows, and the 64 face rows alone).
Every rho is the fp32 reference's own figure, measured on the CPU (test_recorded_rho_is_the_reference_s):

    rho, CPU reference   values      ds_dpoints B=1 / B=3
    H3 sorted            2.765e-07   8.972e-06 / 1.046e-05
    H3 shuffled          4.355e-07   1.016e-05 / 1.063e-05
    H2_22 sorted         2.287e-07   7.559e-06 / 8.385e-06
    H2_22 shuffled       2.334e-07   7.500e-06 / 6.561e-06
    H2_32 sorted         1.572e-07   6.318e-06 / 6.970e-06
    H2_32 shuffled       1.268e-07   6.335e-06 / 6.571e-06

The forward has no sum across threads (include/dpr.h: "values[p, b] has the same bits wherever the point ..."): the
values of a cloud and of the same cloud with its rows permuted agree bit for bit under the permutation.  The sorted
and the shuffled input hold other (point, body) pairs, so each is permuted into the other's regime: the sorted input
by a random permutation (every wave gathers its poses per lane), the shuffled input by the stable sort of its labels
(the waves of one body load their pose with scalar loads).

The pullback runs on atomic, on tiled with max_pose_group 0, 1 and 2 (groups of 2 + 1) and on auto, which
dpr_resolve_algo_sample_smooth_bodies answers with tiled for H3 and atomic for the 2-D inputs (asserted), each with
the drawn ds_dvalues and with NaN in ds_dvalues of every (p, b) the reference rejects by 1e-3 of a cell or more, of
the dropped rows and of the NaN / Inf rows (`poisoned`); the reference never reads those
(test_the_reference_ignores_ds_dvalues_of_rejected_and_dropped_points).

Observed on an MI355X (the tests print them; fp32, the bound m = M_FACTOR rho in brackets):

    values, max |got - ref64| / E     B=1 / B=3
    H3 sorted        2.79e-07 / 2.79e-07 (1.11e-06)    H3 shuffled       2.79e-07 / 3.61e-07 (1.74e-06)
    H2_22 sorted     2.58e-07 / 2.58e-07 (9.15e-07)    H2_22 shuffled    2.58e-07 / 2.58e-07 (9.33e-07)
    H2_32 sorted     1.85e-07 / 1.94e-07 (6.29e-07)    H2_32 shuffled    1.18e-07 / 1.94e-07 (5.07e-07)
    every rejected or dropped (p, b): 0; the permuted cloud: 0 values change their bits, both dtypes.

    ds_dpoints, max |got - ref64| / max |ref64|, B=1 / B=3 -- the same figures on every algorithm (one point kernel)
    and with NaN in ds_dvalues
    H3 sorted       8.91e-06 (3.59e-05) / 1.03e-05 (4.19e-05)   H3 shuffled      1.06e-05 (4.06e-05) / 1.04e-05 (4.25e-05)
    H2_22 sorted    8.53e-06 (3.02e-05) / 8.75e-06 (3.35e-05)   H2_22 shuffled   1.52e-05 (3.00e-05) / 1.11e-05 (2.62e-05)
    H2_32 sorted    7.78e-06 (2.53e-05) / 7.86e-06 (2.79e-05)   H2_32 shuffled   6.34e-06 (2.53e-05) / 7.32e-06 (2.63e-05)
    the 64 cell-face points alone: at most 4.13e-06; dropped and NaN / Inf rows: 0; fp64: at most 2.8e-14 everywhere.

Mutation record: the seven mutants of tests/test_smooth_bodies_hard_gpu.py's docstring, each run once against this
module as well.  Failed here first:
  1 load_body_pose always scalar                   values_one_by_one[H3-sorted-1-float64]: values against the reference,
                                                    2.6 % off
  2 k_smooth_bodies_keys: the tile from image b0   pullback_element_by_element[H3-sorted-3-tiled-0-float64]:
                                                    ds_dimage[.., 1], 85 % off (48 cases pass before: atomic, and B = 1)
  3 k_smooth_bodies_tile: `l < e[d] + 1`           tiled_image_planes_are_the_tiled_splat_of_ds_dvalues[H3-sorted-
                                                    float64]: plane 0, 14 % off (the splat side is the mutant's)
  5 k_sample_smooth_bodies_tile reads              pullback_element_by_element[H3-sorted-3-tiled-0-float64]:
    `ds_dvalues + b0 * P`                           ds_dimage[.., 1], 143 % off
Mutants 4 and 7 (forward mode) do not touch this family.  Mutant 6 (k_sample_smooth_bodies_bwd keeps `tab[i]` after
the flush) passes this module: 587 and 157 blocks of points make three slices of one image each, so no table outlives
an image; tests/test_smooth_bodies_ranges_gpu.py (slices of 65 images) kills it.
"""
import functools

import numpy as np
import pytest
import torch

import dpr_amd
from tests import sample_smooth_bodies_reference as SBR
from tests.test_parity_gpu import assert_close, tol
from tests.test_sample_smooth_hard_gpu import image_to_dev, sample_data, value_budget, values_to_dev
from tests.test_smooth_bodies_hard_gpu import FILL, ORDERS, bodies_input, body_to_dev, hard_cells, subsets
from tests.test_smooth_hard_gpu import DTYPES, INPUTS, M_FACTOR, N_BAD, N_FACE, coords, frozen, to

gpu = pytest.mark.gpu

FIELDS = ("image", "points", "rotation", "translation")
VARIANTS = [("atomic", 0), ("tiled", 0), ("tiled", 1), ("tiled", 2), ("auto", 0)]  # algo, max_pose_group
AUTO = {"H3": "tiled", "H2_22": "atomic", "H2_32": "atomic"}  # what `auto` is for the pullback (asserted below)
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "sorted", "values"): 2.7654e-07,
    ("H3", "sorted", "points", 1): 8.9722e-06,
    ("H3", "sorted", "points", 3): 1.0463e-05,
    ("H3", "shuffled", "values"): 4.3547e-07,
    ("H3", "shuffled", "points", 1): 1.0160e-05,
    ("H3", "shuffled", "points", 3): 1.0627e-05,
    ("H2_22", "sorted", "values"): 2.2869e-07,
    ("H2_22", "sorted", "points", 1): 7.5590e-06,
    ("H2_22", "sorted", "points", 3): 8.3849e-06,
    ("H2_22", "shuffled", "values"): 2.3335e-07,
    ("H2_22", "shuffled", "points", 1): 7.4998e-06,
    ("H2_22", "shuffled", "points", 3): 6.5612e-06,
    ("H2_32", "sorted", "values"): 1.5721e-07,
    ("H2_32", "sorted", "points", 1): 6.3179e-06,
    ("H2_32", "sorted", "points", 3): 6.9697e-06,
    ("H2_32", "shuffled", "values"): 1.2677e-07,
    ("H2_32", "shuffled", "points", 1): 6.3354e-06,
    ("H2_32", "shuffled", "points", 3): 6.5713e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ the references (computed once)
@functools.lru_cache(maxsize=None)
def reference_values(name, order, dtype=np.float64):
    """(P, 3); column b does not depend on the batch"""
    c, s = bodies_input(name, order), sample_data(name)
    with np.errstate(invalid="ignore"):
        v = SBR.sample(s.image, c.points, c.body, c.rot, c.trans, dtype=dtype)
    assert np.all(np.isfinite(v))
    return frozen(v)


@functools.lru_cache(maxsize=None)
def reference_pullback(name, order, B, dtype=np.float64):
    c, s = bodies_input(name, order), sample_data(name)
    with np.errstate(invalid="ignore"):
        pb = SBR.sample_pullback(s.dv[:, :B], s.image[..., :B], c.points, c.body, c.rot[:B], c.trans[:B], dtype=dtype)
    assert all(np.all(np.isfinite(x)) for x in pb)
    frozen(*pb)
    return pb


@functools.lru_cache(maxsize=None)
def budget(name, order):
    """(E[p, b], accepted[p, b]): value_budget per body subset under the body's poses"""
    c, s = bodies_input(name, order), sample_data(name)
    E, acc = np.zeros((c.P, c.B)), np.zeros((c.P, c.B), bool)
    for k, idx in subsets(c):
        E[idx], acc[idx] = value_budget(c.grid, c.points[idx], c.rot[:, k], c.trans[:, k], s.image)
    assert np.array_equal(acc, hard_cells(name, order)[0])
    return frozen(E, acc)


def measured_rho(name, order):
    """{key: rho} of the CPU reference, the keys of RHO."""
    E, acc = budget(name, order)
    v64, v32 = reference_values(name, order), reference_values(name, order, np.float32).astype(np.float64)
    assert not v32[~acc].any(), "the fp32 reference accepts a point that the fp64 reference rejects"
    assert np.all(E[acc] > 0)
    r = {(name, order, "values"): float((np.abs(v32 - v64)[acc] / E[acc]).max())}
    for B in (1, 3):
        p64, p32 = reference_pullback(name, order, B)[1], reference_pullback(name, order, B, np.float32)[1]
        r[(name, order, "points", B)] = float(np.abs(p32.astype(np.float64) - p64).max() / np.abs(p64).max())
    return r


@functools.lru_cache(maxsize=None)
def poisoned(name, order):
    """(P, 3) bool, the (p, b) whose ds_dvalues the tests set to NaN: the fp64 reference rejects (p, b) by at least
    1e-3 of a cell on some axis (far above the rounding of an fp32 coordinate), or the point is dropped, or it is one
    of the five with NaN / Inf coordinates."""
    c = bodies_input(name, order)
    n = np.asarray(c.grid, np.float64)
    far = np.zeros((c.P, c.B), bool)
    for k, idx in subsets(c):
        for b in range(c.B):
            co = coords(c.grid, c.points[idx], c.rot[b, k], c.trans[b, k])
            with np.errstate(invalid="ignore"):
                far[idx, b] = np.any((co < -1 - 1e-3) | (co > n + 1 + 1e-3), axis=1)
    far[c.dropped] = True
    far[-N_BAD:] = True
    return frozen(far)


def dev_args(c, s, tdt, dev, B, rows=slice(None)):
    """[image, points, body, rotation, translation] of the first B images"""
    return [image_to_dev(s.image[..., :B], tdt, dev), to(c.points[rows], tdt, dev), body_to_dev(c, dev)[rows],
            to(c.rot[:B], tdt, dev), to(c.trans[:B], tdt, dev)]


def pullback(dv, args, c, algo, group):
    """sample_smooth_bodies_pullback_ into buffers pre-filled with 7.5 (sorted) or NaN (shuffled)"""
    img, pts, _body, rot, _trans = args
    B, tdt, dev = rot.shape[0], pts.dtype, pts.device
    full = lambda *shape: torch.full(shape, FILL[c.order], dtype=tdt, device=dev)
    bufs = dict(ds_dimage=dpr_amd.empty_grid(c.grid, B, tdt, dev).fill_(FILL[c.order]), ds_dpoints=full(c.P, c.n_in),
                ds_drotation=full(B, c.K, c.n_in, c.n_out).transpose(-1, -2), ds_dtranslation=full(B, c.K, c.n_out))
    kw = dict(max_pose_group=group) if group else {}
    pb = dpr_amd.sample_smooth_bodies_pullback_(dv, *args, algo=algo, **bufs, **kw)
    for f, x in zip(FIELDS, pb):
        assert x.data_ptr() == bufs["ds_d" + f].data_ptr(), f"ds_d{f} is not the caller's buffer"
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    return pb


# ------------------------------------------------------------------ the CPU side
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_recorded_rho_is_the_reference_s(name, order):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 1 %."""
    for key, rho in measured_rho(name, order).items():
        print(f"rho {key}: {rho:.4e}")
        assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
        assert abs(RHO[key] - rho) <= 0.01 * rho, f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_the_reference_ignores_ds_dvalues_of_rejected_and_dropped_points(name, order):
    """At least 20 rejected (p, b) per image and every dropped row; the reference gives the same results with NaN,
    with 0 and with the drawn ds_dvalues there (the 2-D inputs: one pullback more)."""
    c, s = bodies_input(name, order), sample_data(name)
    far, (_E, acc) = poisoned(name, order), budget(name, order)
    print(f"{name} {order}: poisoned (p, b) per image {far.sum(axis=0)}, {len(c.dropped)} dropped rows among them")
    assert np.all(far.sum(axis=0) >= 20 + len(c.dropped)) and far[c.dropped].all() and not (far & acc).any()
    if name != "H3":
        with np.errstate(invalid="ignore"):
            for fill in (0.0, np.nan):
                other = SBR.sample_pullback(np.where(far, fill, s.dv), s.image, c.points, c.body, c.rot, c.trans)
                for a, e in zip(other, reference_pullback(name, order, 3)):
                    assert np.array_equal(a, e)


# ------------------------------------------------------------------ 1 values, one by one
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_values_one_by_one(dev, name, order, B, npdt, tdt):
    c, s = bodies_input(name, order), sample_data(name)
    ref64 = reference_values(name, order)[:, :B]
    E, acc = (a[:, :B] for a in budget(name, order))
    v = dpr_amd.sample_smooth_bodies(*dev_args(c, s, tdt, dev, B))
    assert tuple(v.shape) == (c.P, B) and v.dtype == tdt and v.t().is_contiguous()
    got = v.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite values"
    assert_close(v, ref64.astype(npdt), tol(npdt, "points"), f"{name} {order} B={B}")
    bad = ~acc & (got != 0)
    assert not bad.any(), f"{int(bad.sum())} rejected or dropped (p, b) have a value; first {tuple(np.argwhere(bad)[0])}"
    assert not got[c.dropped].any()
    if npdt == np.float32:
        m = M_FACTOR * RHO[(name, order, "values")]
        d = np.abs(got - ref64)
        ratio = np.where(acc, d / np.where(acc, E, 1.0), 0.0)
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{name} {order} B={B}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
        over = d > m * E
        assert not over.any(), f"(p, b) = {worst}: |got - ref64| = {d[worst]:.3e} > {m:.3e} * E = " \
            f"{m * E[worst]:.3e} ({int(over.sum())} values over the bound)"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_values_do_not_depend_on_the_order_of_the_cloud(dev, name, order, npdt, tdt):
    """The cloud with its rows permuted into the other regime of load_body_pose (see the module docstring): the
    same bits under the permutation, and the same bits run to run."""
    c, s = bodies_input(name, order), sample_data(name)
    if order == "sorted":
        perm = np.random.default_rng(12).permutation(c.P)
    else:
        perm = np.argsort(c.body, kind="stable")
        runs = c.body[perm]
        assert np.all(np.diff(runs) >= 0) and any(len(np.unique(runs[i:i + 256])) == 1 for i in range(0, c.P, 256))
    assert not np.array_equal(perm, np.arange(c.P))
    v = dpr_amd.sample_smooth_bodies(*dev_args(c, s, tdt, dev, c.B))
    assert torch.equal(v, dpr_amd.sample_smooth_bodies(*dev_args(c, s, tdt, dev, c.B))), "two runs differ"
    w = dpr_amd.sample_smooth_bodies(*dev_args(c, s, tdt, dev, c.B, perm))
    moved = v[torch.as_tensor(perm, device=dev)]
    differ = int((moved != w).sum())
    assert differ == 0, f"{differ} values change their bits with the order of the cloud"
    assert float(w.abs().max()) > 0


# ------------------------------------------------------------------ 2 the pullback, element by element
def check_hard_pullback(pb, name, order, B, npdt, what):
    c = bodies_input(name, order)
    ref = reference_pullback(name, order, B)
    for b in range(B):
        assert_close(pb.image[..., b], ref[0][..., b].astype(npdt), tol(npdt, "out"), f"{what}ds_dimage[.., {b}]")
        for k in range(c.K):
            rtol = tol(npdt, "pose")
            assert_close(pb.rotation[b, k], ref[2][b, k].astype(npdt), rtol, f"{what}ds_drotation[{b}, {k}]")
            assert_close(pb.translation[b, k], ref[3][b, k].astype(npdt), rtol, f"{what}ds_dtranslation[{b}, {k}]")
    got, e = pb.points.cpu().numpy().astype(np.float64), ref[1]
    scale = np.abs(e).max()
    m = M_FACTOR * RHO[(name, order, "points", B)] if npdt == np.float32 else tol(npdt, "points")
    d = np.abs(got - e).max(axis=1)
    faces = np.arange(c.P - N_BAD - N_FACE, c.P - N_BAD)
    print(f"{what}{np.dtype(npdt).name} ds_dpoints: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
          f"(m = {m:.3e}); face points {d[faces].max() / scale:.3e}")
    if npdt == np.float32:
        assert d.max() <= m * scale, f"{what}ds_dpoints: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} " \
            f"at point {int(d.argmax())}"
    else:
        assert_close(pb.points, e, tol(npdt, "points"), f"{what}ds_dpoints")
    over = np.nonzero(d[faces] > m * scale)[0]
    assert len(over) == 0, f"{what}ds_dpoints of face point {int(faces[over[0]])}: off by {d[faces][over[0]]:.3e} > " \
        f"{m:.3e} * {scale:.3e}; {len(over)} face points over the bound"
    assert not got[c.dropped].any(), f"{what}ds_dpoints of a dropped point is not 0"
    assert not got[-N_BAD:].any(), f"{what}ds_dpoints of a NaN / Inf point is not 0"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,group", VARIANTS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, order, B, algo, group, npdt, tdt):
    """With the drawn ds_dvalues, and with NaN in ds_dvalues of every rejected and dropped (p, b): nothing may read
    them into a result (a product with a zero weight would)."""
    c, s = bodies_input(name, order), sample_data(name)
    if algo == "auto":
        assert dpr_amd.resolve_algo_sample_smooth_bodies("pullback", c.grid, c.P, B, c.K, c.n_in) == AUTO[name]
    args = dev_args(c, s, tdt, dev, B)
    for dv, note in ((s.dv, ""), (np.where(poisoned(name, order), np.nan, s.dv), "NaN ds_dvalues: ")):
        pb = pullback(values_to_dev(dv[:, :B], tdt, dev), args, c, algo, group)
        check_hard_pullback(pb, name, order, B, npdt, f"{name} {order} {algo} group {group} B={B} {note}")


@pytest.mark.parametrize("name", INPUTS)
def test_auto_pullback_is_what_the_library_answers(name):
    """(CPU)  dpr_resolve_algo_sample_smooth_bodies from the shape alone (the labels are no part of it): the `auto`
    cases of test_pullback_element_by_element run the tiled planes on H3 and the atomic kernel alone in 2-D."""
    c = bodies_input(name, "sorted")
    for B in (1, 3):
        assert dpr_amd.resolve_algo_sample_smooth_bodies("pullback", c.grid, c.P, B, c.K, c.n_in) == AUTO[name]
        assert dpr_amd.resolve_algo_sample_smooth_bodies("sample", c.grid, c.P, B, c.K, c.n_in) == "atomic"


# ------------------------------------------------------------------ 3 the tiled planes are the tiled splat's
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_tiled_image_planes_are_the_tiled_splat_of_ds_dvalues(dev, name, order, npdt, tdt):
    """ds_dimage[.., b] on tiled against raster_smooth_bodies_(algo="tiled") of one image with point weights
    ds_dvalues[:, b], background 0 and out_weight 1, within tol()."""
    c, s = bodies_input(name, order), sample_data(name)
    args = dev_args(c, s, tdt, dev, c.B)
    _img, pts, body, rot, trans = args
    pb = pullback(values_to_dev(s.dv, tdt, dev), args, c, "tiled", 0)
    for b in range(c.B):
        plane = dpr_amd.empty_grid(c.grid, 1, tdt, dev).fill_(FILL[c.order])
        dpr_amd.raster_smooth_bodies_(plane, pts, body, rot[b:b + 1], trans[b:b + 1], None, None,
                                      to(s.dv[:, b], tdt, dev), algo="tiled")
        assert bool(torch.isfinite(plane).all())
        assert_close(pb.image[..., b], plane[..., 0].cpu().numpy(), tol(npdt, "out"), f"{name} {order} plane {b}")
