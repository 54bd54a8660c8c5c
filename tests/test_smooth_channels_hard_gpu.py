"""The smooth splat with C weights per point (csrc/dpr_smooth_channels.hip) in the hard regimes: the clustered inputs
of tests/test_smooth_hard_gpu.py with cell-face and NaN / Inf points, cell by cell and element by element; the
key-bit and small-grid edges of the tiled forward; the pullback of a batch on either side of the pose-slice
threshold; mass.

Every expectation is tests/smooth_channels_reference.py (`SCR`: tests/smooth_reference.py channel by channel) in fp64
on inputs rounded to fp32 once.  The weights are those of tests/test_smooth_channels_gpu.py (`_weights`): sixteen
channels in [0.5, 1.5], channel 1 all zero, channel 2 of both signs; every background is non-zero.

3a  forward: C = 4 (the 4-channel kernels, whole chunks of the tiled forward's 2 channels per workgroup) and C = 5
(the 16-channel kernels, a last chunk of one channel) on H3 / H2_22 / H2_32, C = 16 on H2_22 alone (an H3 reference
of 16 channels takes minutes on the CPU).  |got - ref64| <= M_FACTOR rho E_c on every cell of every plane (c, b), E_c
the budget of tests/test_smooth_hard_gpu.py (`budget_of`) with channel c's weights and background, rho the largest
|ref32 - ref64| / E_c over the channels.  3b  pullback, C = 5 (H3: C = 3, the 4-channel kernel with a half-filled
bound; the single-pose references of five channels of H3 take 40 s on the CPU): ds_dpoints and all columns of
ds_dpoint_weight, max |got - ref64| <= M_FACTOR rho max |ref64|.  Each rho is the fp32 reference's own figure,
measured on the CPU (test_recorded_rho_is_the_reference_s):

    rho, CPU reference    forward, per cell (5 ch. / 16 ch.)    ds_dpoints B=1 / B=3    ds_dpoint_weight B=1 / B=3
    H3 (pullback: C = 3)  1.373e-06                             9.227e-06 / 8.297e-06   9.864e-06 / 7.399e-06
    H2_22                 9.644e-07 / 9.644e-07                 1.290e-05 / 9.238e-06   6.458e-06 / 7.681e-06
    H2_32                 1.580e-06                             6.233e-06 / 7.665e-06   5.918e-06 / 4.982e-06

3c  `edge_case` on every EDGE_GRIDS entry with C = 3 (a half-filled last chunk).  3d  (2,2), (64, 64), C = 3,
B = 3: P = 524 033 (2 048 blocks: one slice, one thread adds the poses and stores) and P = 523 776 (2 046 blocks: two
slices, atomics onto zero).  3e  mass of `interior_cloud`, C = 5, the derived bound of
test_mass_of_an_interior_cloud per plane (c, b).

Observed on an MI355X (the tests print them):
    forward, fp32: max |got - ref64| / E (m), atomic and tiled alike     B=1, C = 4 / 5          B=3, C = 4 / 5
    H3 (5.49e-06)                                                          9.95e-08 / 1.18e-07     6.84e-07 / 6.84e-07
    H2_22 (3.86e-06)                                                       8.61e-08 / 8.89e-08     1.06e-06 / 1.06e-06
    H2_32 (6.32e-06)                                                       9.25e-08 / 9.27e-08     7.30e-07 / 7.30e-07
    H2_22, C = 16 (3.86e-06): 8.89e-08 (B=1), 1.12e-06 (B=3)
    pullback, fp32: max |got - ref64| / max |ref64| (m)    ds_dpoints B=1 / B=3               ds_dpoint_weight B=1 / B=3
    H3      9.27e-06 (3.69e-05) / 8.71e-06 (3.32e-05)      9.86e-06 (3.95e-05) / 9.41e-06 (2.96e-05)
    H2_22   1.29e-05 (5.16e-05) / 1.95e-05 (3.70e-05)      6.52e-06 (2.58e-05) / 9.73e-06 (3.07e-05)
    H2_32   6.24e-06 (2.49e-05) / 1.09e-05 (3.07e-05)      5.99e-06 (2.37e-05) / 7.56e-06 (1.99e-05)
    (B = 3: the atomics' arrival order moves the last digits.)  The 64 face points alone: at most 6.6e-06; fp64: at
    most 1.7e-14 everywhere.
    mass, fp64: off by at most 7.3e-12 against bounds of 2.5e-08 .. 6.0e-06.

Mutation record (scratch builds of libdpr, one MI355X run of this module each; both mutants keep every access inside
the buffers: a wrong channel offset reads columns 0 .. 1 of point_weight, an overwritten sum writes where the sum
is written):
  k_smooth_ch_tile loads its chunk's weights     forward_cell_by_cell[H3-4-tiled-1-float64]: channel 2 against the
  from channel 0 (`c0` -> 0)                     reference norm-wise, 100 % off (atomic passes before)
  k_smooth_ch_bwd `acc_pw[c] = W * ps.ow`        pullback_of_a_batch_at_the_slice_threshold[524033-float64]:
  for `+=`                                       ds_dpoint_weight 71 % off; the 128 cases before it pass, 3b with B = 3
                                                 among them: 157 or 587 blocks of points put each of three poses in a
                                                 slice of its own, where `=` and `+=` are the same -- 3d is the one
                                                 place where a slice holds several poses and the points' sums are stored
Argued, not run: a wider LDS window or a dropped `c < gd.n[d]` test writes past the LDS array or the plane.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_channels_reference as SCR
from tests import smooth_reference as SR
from tests.test_parity_gpu import assert_close, grid_to_dev, tol
from tests.test_smooth_hard_gpu import (DTYPES, EDGE_CASES, INPUTS, LARGE_P, M_FACTOR, N_BAD, N_FACE, budget_of,
                                        edge_case, far_cells, frozen, interior_cloud, large_case, pose_slice_count,
                                        r32, smooth_data, smooth_input, to)

gpu = pytest.mark.gpu

FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")
CMAX = {"H3": 5, "H2_22": 16, "H2_32": 5}  # the channels a reference is computed for
C_PULLBACK = {"H3": 3, "H2_22": 5, "H2_32": 5}  # (H3: three channels, its five take 40 s on the CPU)
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "out", 5): 1.3727e-06,
    ("H3", "points", 1): 9.2274e-06,
    ("H3", "point_weight", 1): 9.8643e-06,
    ("H3", "points", 3): 8.2972e-06,
    ("H3", "point_weight", 3): 7.3987e-06,
    ("H2_22", "out", 5): 9.6440e-07,
    ("H2_22", "out", 16): 9.6440e-07,
    ("H2_22", "points", 1): 1.2902e-05,
    ("H2_22", "point_weight", 1): 6.4577e-06,
    ("H2_22", "points", 3): 9.2376e-06,
    ("H2_22", "point_weight", 3): 7.6810e-06,
    ("H2_32", "out", 5): 1.5801e-06,
    ("H2_32", "points", 1): 6.2326e-06,
    ("H2_32", "point_weight", 1): 5.9181e-06,
    ("H2_32", "points", 3): 7.6654e-06,
    ("H2_32", "point_weight", 3): 4.9822e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def weights(rng, P, C):
    from tests.test_smooth_channels_gpu import _weights
    return r32(_weights(rng, P, C))


def backgrounds(rng, B, C):
    bg = r32(rng.normal(size=(B, C)))
    bg[np.abs(bg) < 0.05] = 0.05
    return bg


def dev_args(c, tdt, dev, C, B, keep=slice(None)):
    """points, rotation, translation, point_weight, background, out_weight"""
    t = lambda a: to(a, tdt, dev)
    return [t(c.points[keep]), t(c.rot[:B]), t(c.trans[:B]), t(c.pw[keep, :C]), t(c.bg[:B, :C]), t(c.ow[:B])]


def grads(pb):
    return (pb.points, pb.rotation, pb.translation, pb.background, pb.out_weight, pb.point_weight)


def combine_poses(parts, B, dtype):
    """The gradients of the first B poses from single-pose ones, `parts[c][b]`: the rows of a pose are its own, and
    the point gradients add pose by pose in index order onto zero, as tests/smooth_reference.py adds them."""
    per_channel = []
    for ch in parts:
        d_pts, d_pw = np.zeros_like(ch[0][0]), np.zeros_like(ch[0][5])
        for b in range(B):
            d_pts, d_pw = d_pts + ch[b][0], d_pw + ch[b][5]
        per_channel.append((d_pts,) + tuple(np.concatenate([ch[b][i] for b in range(B)]) for i in (1, 2, 3, 4))
                           + (d_pw,))
    out = SCR.combine(per_channel)
    assert all(x.dtype == dtype for x in out)
    return out


# ------------------------------------------------------------------ the hard inputs with sixteen channels
@functools.lru_cache(maxsize=None)
def hard_case(name):
    h, s = smooth_input(name), smooth_data(name)
    rng = np.random.default_rng(6100 + len(name) + h.n_in)
    c = SimpleNamespace(name=name, n_in=h.n_in, n_out=h.n_out, grid=h.grid, P=h.P, B=h.B, points=h.points, rot=h.rot,
                        trans=h.trans, ow=s.ow, pw=weights(rng, h.P, 16), bg=backgrounds(rng, h.B, 16),
                        g=r32(rng.normal(size=h.grid + (C_PULLBACK[name], h.B))))
    assert np.all(c.bg != 0) and not c.pw[:, 1].any() and c.pw[:, 2].min() < 0 < c.pw[:, 2].max()
    frozen(c.pw, c.bg, c.g)
    return c


@functools.lru_cache(maxsize=None)
def reference_out(name, dtype=np.float64):
    """grid + (CMAX[name], 3)"""
    c = hard_case(name)
    C = CMAX[name]
    with np.errstate(invalid="ignore"):
        out = SCR.raster_smooth_channels(c.grid, c.points, c.rot, c.trans, c.pw[:, :C], c.bg[:, :C], c.ow, dtype=dtype)
    assert np.all(np.isfinite(out))
    return frozen(out)


@functools.lru_cache(maxsize=None)
def budget(name):
    """E of tests/test_smooth_hard_gpu.py for every channel: grid + (CMAX[name], 3)"""
    c = hard_case(name)
    E = np.stack([budget_of(c.grid, c.points, c.rot, c.trans, c.bg[:, ch], c.ow, c.pw[:, ch])
                  for ch in range(CMAX[name])], axis=-2)
    assert np.all(E > 0)
    return frozen(E)


@functools.lru_cache(maxsize=None)
def pose_parts(name, dtype=np.float64):
    """parts[c][b]: the single-channel, single-pose gradients of channel c < C_PULLBACK[name] and pose b"""
    c = hard_case(name)
    with np.errstate(invalid="ignore"):
        parts = [[SR.raster_pullback_smooth(c.g[..., ch, b:b + 1], c.points, c.rot[b:b + 1], c.trans[b:b + 1],
                                            c.ow[b:b + 1], c.pw[:, ch], dtype=dtype) for b in range(c.B)]
                 for ch in range(C_PULLBACK[name])]
    assert all(np.all(np.isfinite(x)) for ch in parts for p in ch for x in p)
    return parts


@functools.lru_cache(maxsize=None)
def reference_pullback(name, B, dtype=np.float64):
    pb = combine_poses(pose_parts(name, dtype), B, dtype)
    frozen(*pb)
    return pb


def measured_rho(name):
    ratio = np.abs(reference_out(name, np.float32).astype(np.float64) - reference_out(name)) / budget(name)
    r = {(name, "out", 5): float(ratio[..., :5, :].max())}
    if CMAX[name] == 16:
        r[(name, "out", 16)] = float(ratio.max())
    for B in (1, 3):
        p64, p32 = reference_pullback(name, B), reference_pullback(name, B, np.float32)
        for field, i in (("points", 0), ("point_weight", 5)):
            r[(name, field, B)] = float(np.abs(p32[i].astype(np.float64) - p64[i]).max() / np.abs(p64[i]).max())
    return r


@pytest.mark.parametrize("name", INPUTS)
def test_recorded_rho_is_the_reference_s(name):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 1 %."""
    for key, rho in measured_rho(name).items():
        print(f"rho {key}: {rho:.4e}")
        assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
        assert abs(RHO[key] - rho) <= 0.01 * rho, f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@pytest.mark.parametrize("name", INPUTS)
def test_channel_inputs_reach_the_regimes(name):
    """(CPU)  The cloud's regimes are asserted by tests/test_smooth_hard_gpu.py::test_hard_inputs_reach_the_regimes;
    here: the zero channel's planes are their background, channel 2 deposits with both signs, the far cells hold the
    background on every plane and the combined single-pose gradients are the batch's."""
    c, out, far = hard_case(name), reference_out(name), far_cells(name)
    assert np.array_equal(out[..., 1, :], np.broadcast_to(c.bg[:, 1], out[..., 1, :].shape))
    d = out[..., 2, :] - c.bg[:, 2]
    assert d.min() < 0 < d.max()
    mask = np.broadcast_to(far[..., None, :], out.shape)
    assert np.array_equal(out[mask], np.broadcast_to(c.bg[:, :CMAX[name]].T, out.shape)[mask]) and mask.any()
    if name == "H2_22":  # (the smallest input: the batch's reference in one call, once)
        with np.errstate(invalid="ignore"):
            whole = SCR.raster_pullback_smooth_channels(c.g, c.points, c.rot, c.trans, c.pw[:, :C_PULLBACK[name]], c.ow)
        for f, a, e in zip(FIELDS, reference_pullback(name, 3), whole):
            assert np.array_equal(a, e), f


# ------------------------------------------------------------------ 3a the forward, cell by cell
FORWARD = [(name, C) for name in INPUTS for C in (4, 5)] + [("H2_22", 16)]


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("name,C", FORWARD)
def test_forward_cell_by_cell(dev, name, C, algo, B, npdt, tdt):
    c = hard_case(name)
    ref64 = reference_out(name)[..., :C, :B]
    out = dpr_amd.raster_smooth_channels(c.grid, *dev_args(c, tdt, dev, C, B), algo=algo)
    assert tuple(out.shape) == c.grid + (C, B) and out.dtype == tdt
    raw = out.cpu().numpy()
    got = raw.astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out"
    what = f"{name} C={C} {algo} B={B}"
    for ch in range(C):
        assert_close(out[..., ch, :], ref64[..., ch, :].astype(npdt), tol(npdt, "out"), f"{what} channel {ch}")
    if npdt == np.float32:
        E = budget(name)[..., :C, :B]
        m = M_FACTOR * RHO[(name, "out", 16 if C == 16 else 5)]
        ratio = np.abs(got - ref64) / E
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{what}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
        assert ratio.max() <= m, f"cell, c, b = {worst}: |got - ref64| = {abs(got[worst] - ref64[worst]):.3e} > " \
            f"{m:.3e} * E = {m * E[worst]:.3e} ({int((ratio > m).sum())} cells over the bound)"
    want = np.broadcast_to(c.bg[:B, :C].T.astype(npdt), raw.shape)
    assert np.array_equal(raw[..., 1, :], want[..., 1, :]), f"{what}: the zero channel is not its background"
    far = np.broadcast_to(far_cells(name)[..., None, :B], raw.shape)
    bad = far & (raw != want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(far.sum())} far cells are not the background; " \
        f"first {tuple(int(v) for v in np.argwhere(bad)[0])}"


# ------------------------------------------------------------------ 3b the pullback, element by element
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, B, npdt, tdt):
    c, C = hard_case(name), C_PULLBACK[name]
    ref = reference_pullback(name, B)
    g = grid_to_dev(c.g[..., :B].astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_channels_(g, *dev_args(c, tdt, dev, C, B))
    assert tuple(pb.point_weight.shape) == (c.P, C) and tuple(pb.background.shape) == (B, C)
    for f, x in zip(FIELDS, grads(pb)):
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    for f, kind, a, e in zip(FIELDS, KINDS, grads(pb), ref):
        if kind == "pose" or npdt == np.float64:
            assert_close(a, e.astype(npdt), tol(npdt, kind), f"{name} B={B} {f}")
    faces = np.arange(c.P - N_BAD - N_FACE, c.P - N_BAD)
    for f, i in (("points", 0), ("point_weight", 5)):
        got, e = grads(pb)[i].cpu().numpy().astype(np.float64), ref[i]
        scale = np.abs(e).max()
        m = M_FACTOR * RHO[(name, f, B)] if npdt == np.float32 else tol(npdt, "points")
        d = np.abs(got - e)
        print(f"{name} B={B} {np.dtype(npdt).name} ds_d{f}: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
              f"(m = {m:.3e}); face points {d[faces].max() / scale:.3e}")
        if npdt == np.float32:
            assert d.max() <= m * scale, f"ds_d{f}: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} at " \
                f"(point, column) {np.unravel_index(int(d.argmax()), d.shape)}"
        row = d.max(axis=1)[faces]  # the cell-face points one by one
        over = np.nonzero(row > m * scale)[0]
        assert len(over) == 0, f"ds_d{f} of face point {int(faces[over[0]])} ({c.points[faces[over[0]]]}): off by " \
            f"{row[over[0]]:.3e} > {m:.3e} * {scale:.3e}; {len(over)} face points over the bound"
    assert not bool((pb.points[-N_BAD:] != 0).any()), "ds_dpoints of a NaN / Inf point is not 0"
    assert not bool((pb.point_weight[-N_BAD:] != 0).any()), "ds_dpoint_weight of a NaN / Inf point, some column"
    if B == 1:  # one thread per point, plain stores: the other rows do not know of the five
        keep = slice(0, c.P - N_BAD)
        pc = dpr_amd.raster_pullback_smooth_channels_(g, *dev_args(c, tdt, dev, C, B, keep))
        assert torch.equal(pb.points[keep], pc.points), "ds_dpoints of the other points"
        assert torch.equal(pb.point_weight[keep], pc.point_weight), "ds_dpoint_weight of the other points"


# ------------------------------------------------------------------ 3c key bits and small grids
@functools.lru_cache(maxsize=None)
def edge_channels(n_in, grid):
    e = edge_case(n_in, grid)
    rng = np.random.default_rng(6300 + n_in + sum(grid))
    C = 3
    c = SimpleNamespace(grid=grid, P=e.P, B=e.B, points=e.points, rot=e.rot, trans=e.trans, ow=e.ow,
                        pw=weights(rng, e.P, C), bg=backgrounds(rng, e.B, C), g=r32(rng.normal(size=grid + (C, e.B))))
    with np.errstate(invalid="ignore"):
        c.out = SCR.raster_smooth_channels(grid, c.points, c.rot, c.trans, c.pw, c.bg, c.ow)
        c.pb = SCR.raster_pullback_smooth_channels(c.g, c.points, c.rot, c.trans, c.pw, c.ow)
    assert np.all(np.isfinite(c.out)) and all(np.all(np.isfinite(x)) for x in c.pb)
    frozen(c.pw, c.bg, c.g, c.out, *c.pb)
    return c


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid", EDGE_CASES)
def test_key_bit_and_small_grid_edges(dev, n_in, n_out, grid, npdt, tdt):
    c, C = edge_channels(n_in, grid), 3
    args = dev_args(c, tdt, dev, C, c.B)
    need = dpr_amd.workspace_bytes_smooth_channels("raster", grid, c.P, c.B, n_in, C, tdt, "tiled")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tiled = dpr_amd.raster_smooth_channels(grid, *args, algo="tiled", workspace=ws)
    atomic = dpr_amd.raster_smooth_channels(grid, *args, algo="atomic")
    assert tuple(tiled.shape) == grid + (C, c.B)
    assert bool(torch.isfinite(tiled).all()) and bool(torch.isfinite(atomic).all())
    for ch in range(C):
        for b in range(c.B):  # plane by plane: a plane must not hide in another's norm
            e = c.out[..., ch, b].astype(npdt)
            assert_close(tiled[..., ch, b], e, tol(npdt, "out"), f"{grid} tiled, plane ({ch}, {b})")
            assert_close(atomic[..., ch, b], e, tol(npdt, "out"), f"{grid} atomic, plane ({ch}, {b})")
    assert bool((tiled[..., 1, :] == atomic[..., 1, :]).all()), "the zero channel"
    pb = dpr_amd.raster_pullback_smooth_channels_(grid_to_dev(c.g.astype(npdt), dev), *args)
    for f, kind, a, e in zip(FIELDS, KINDS, grads(pb), c.pb):
        assert bool(torch.isfinite(a).all()), f"non-finite ds_d{f}"
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"{grid} {f}")
    for ch in range(C):
        assert_close(pb.point_weight[:, ch], c.pb[5][:, ch].astype(npdt), tol(npdt, "points"),
                     f"{grid} ds_dpoint_weight[:, {ch}]")
    assert not bool((pb.points[-6:] != 0).any()) and not bool((pb.point_weight[-6:] != 0).any())


# ------------------------------------------------------------------ 3d one slice, several poses
def test_large_clouds_sit_on_both_sides_of_the_slice_threshold():
    assert {P: pose_slice_count(P, 3) for P in LARGE_P} == {524_033: (2048, 1), 523_776: (2046, 2)}


@functools.lru_cache(maxsize=None)
def large_channels():
    e = large_case(2)
    rng = np.random.default_rng(6400)
    C, B, P = 3, 3, max(LARGE_P)
    c = SimpleNamespace(grid=e.grid, B=B, points=e.points, rot=e.rot[:B], trans=e.trans[:B], ow=e.ow[:B],
                        pw=weights(rng, P, C), bg=backgrounds(rng, B, C), g=r32(rng.normal(size=e.grid + (C, B))))
    frozen(c.pw, c.bg, c.g)
    return c


@functools.lru_cache(maxsize=None)
def large_reference(P):
    """three single-channel pullbacks of the first P points"""
    c = large_channels()
    return SCR.raster_pullback_smooth_channels(c.g, c.points[:P], c.rot, c.trans, c.pw[:P], c.ow)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("P", list(LARGE_P))
def test_pullback_of_a_batch_at_the_slice_threshold(dev, P, npdt, tdt):
    """P = 524 033: one slice holds the three poses, a thread adds them and stores ds_dpoints and the C columns of
    ds_dpoint_weight once (the same bits run to run).  P = 523 776: two slices, atomics onto zero."""
    c, C = large_channels(), 3
    assert pose_slice_count(P, c.B)[1] == LARGE_P[P][1]
    g = grid_to_dev(c.g.astype(npdt), dev)
    args = dev_args(c, tdt, dev, C, c.B, slice(0, P))
    pb = dpr_amd.raster_pullback_smooth_channels_(g, *args)
    ref = large_reference(P)
    for f, kind, a, e in zip(FIELDS, KINDS, grads(pb), ref):
        assert_close(a, e.astype(npdt), tol(npdt, kind), f"P={P} {f}")
    for ch in range(C):
        assert_close(pb.point_weight[:, ch], ref[5][:, ch].astype(npdt), tol(npdt, "points"),
                     f"P={P} ds_dpoint_weight[:, {ch}]")
    if LARGE_P[P][1] == 1:
        again = dpr_amd.raster_pullback_smooth_channels_(g, *args)
        assert torch.equal(pb.points, again.points), "ds_dpoints differs between two runs"
        assert torch.equal(pb.point_weight, again.point_weight), "ds_dpoint_weight differs between two runs"


# ------------------------------------------------------------------ 3e mass
@gpu
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_mass_of_an_interior_cloud(dev, n_in, n_out, algo):
    """fp64, per plane (c, b): |sum out[.., c, b] - G bg_bc - ow_b sum pw_c| <= (3^N P + G) eps (G |bg_bc| +
    |ow_b| sum |pw_c|), the any-order worst case for that many additions; for the zero channel this is the bound of
    its background alone."""
    m, C = interior_cloud(n_in, n_out), 5
    rng = np.random.default_rng(6500 + 10 * n_in + n_out)
    c = SimpleNamespace(points=m.points, rot=m.rot, trans=m.trans, ow=m.ow, pw=weights(rng, m.P, C),
                        bg=backgrounds(rng, m.B, C))
    out = dpr_amd.raster_smooth_channels(m.grid, *dev_args(c, torch.float64, dev, C, m.B), algo=algo)
    total = out.sum(dim=tuple(range(n_out))).cpu().numpy()  # (C, B)
    G = int(np.prod(m.grid))
    eps = float(np.finfo(np.float64).eps)
    for ch in range(C):
        for b in range(m.B):
            want = G * c.bg[b, ch] + c.ow[b] * c.pw[:, ch].sum()
            bound = (3 ** n_out * m.P + G) * eps * (G * abs(c.bg[b, ch]) + abs(c.ow[b]) * np.abs(c.pw[:, ch]).sum())
            print(f"({n_in}, {n_out}) {algo} plane ({ch}, {b}): mass off by {abs(total[ch, b] - want):.3e}, "
                  f"bound {bound:.3e}")
            assert abs(total[ch, b] - want) <= bound, (ch, b, total[ch, b], want, bound)
