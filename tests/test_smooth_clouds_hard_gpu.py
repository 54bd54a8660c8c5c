"""The smooth splat of per-pose clouds (k_smooth_clouds_* of csrc/dpr_smooth.hip) in the hard regimes: clustered clouds
with cell-face and NaN / Inf points cell by cell and element by element, the key bits of a pose group of the tiled
forward (smooth_clouds_fwd_tiled sorts a group of nb poses on ord_key_bits(nb * tiles) bits; the last group of a call
may hold fewer poses and so have other bits), and mass.

Every expectation is tests/smooth_reference.py (`SR`) in fp64, pose by pose on (cloud b, pose b), on inputs rounded
to fp32 once.

2a  Three clouds from each hard input of tests/test_smooth_hard_gpu.py (`smooth_input`): cloud 0 the input; cloud 1
its rows reversed and scaled by 0.9; cloud 2 rolled by 1 000 rows and scaled by 1.1; the six border points of
`smooth_input` stay in front and the 64 cell-face and 5 NaN / Inf points stay the tail of every cloud, unscaled (the
border points of a scaled cloud would leave the border).  Counted on the CPU from the reference's cell choice
(test_clustered_clouds_reach_the_regimes recounts and asserts), per (cloud b, pose b):

    input   tiles   heaviest (pose, tile) run, cloud 0 / 1 / 2   empty tiles       rejected        j0 = -1     j0 = n_0
    H3      405     88 317 / 93 683 / 110 732                    108 / 152 / 108   65 / 57 / 231   3 / 1 / 3   4 / 2 / 1
    H2_22   10      37 937 / 26 668 / 29 658                     0 / 0 / 0         22 / 26 / 66    2 / 1 / 2   3 / 2 / 6
    H2_32   10      38 095 / 34 924 / 20 070                     0 / 0 / 0         21 / 22 / 62    4 / 1 / 1   3 / 5 / 4

The forward is held per cell, |got - ref64| <= M_FACTOR rho E on every cell, E the budget of
tests/test_smooth_hard_gpu.py (`budget_of`) with the weights of (cloud b, pose b), and the point gradients per
element, max |got - ref64| <= M_FACTOR rho max |ref64|; each rho is the fp32 reference's own figure, measured on the
CPU (test_recorded_rho_is_the_reference_s):

    rho, CPU reference    forward, per cell    ds_dpoints    ds_dpoint_weight
    H3                    3.113e-07            9.389e-06     9.163e-06
    H2_22                 7.732e-07            8.600e-06     8.495e-06
    H2_32                 7.356e-07            6.978e-06     6.635e-06

2b  Key bits.  (tiles, B, max_pose_group) -> nb * tiles and bits of the full and of the last group; see KEY_CASES
and test_key_cases_cover_the_key_bit_edges.  2c  Mass of three interior clouds, the derived bound of
test_mass_of_an_interior_cloud.

Observed on an MI355X (the tests print them):
    forward, fp32: max |got - ref64| / E (m), the same on atomic and on tiled with max_pose_group 0 / 1 / 2
    H3 3.35e-07 (1.25e-06)    H2_22 1.59e-06 (3.09e-06)    H2_32 8.33e-07 (2.94e-06)
    pullback, fp32: max |got - ref64| / max |ref64| (m); the 64 face points alone
    H3      ds_dpoints 9.39e-06 (3.76e-05); 2.72e-06    ds_dpoint_weight 1.07e-05 (3.67e-05); 4.47e-06
    H2_22   ds_dpoints 9.57e-06 (3.44e-05); 5.22e-06    ds_dpoint_weight 1.20e-05 (3.40e-05); 3.85e-06
    H2_32   ds_dpoints 8.67e-06 (2.79e-05); 4.89e-06    ds_dpoint_weight 9.63e-06 (2.65e-05); 5.88e-06
    fp64: at most 1.8e-14 everywhere.
    mass, fp64: off by at most 7.3e-12 against bounds of 7.4e-07 .. 6.5e-06.

Mutation record (a scratch build of libdpr, one MI355X run of this module; the start table stays clamped by
ord_cell_range and `q >= count`, so a mis-sorted group shortens or misplaces a walk and never leaves the buffers):
  smooth_clouds_fwd_tiled sorts on bits - 1      forward_cell_by_cell[H3-tiled-0-float64]: plane 0 against the reference
  bits (where bits > 1)                          norm-wise, 0.2 % off (the two atomic cases before it pass).  2b and 2c
                                                 alone, in a second run: key_bits_of_a_group fails 96 of its 102 cases,
                                                 first [(1, 5, 4)-float64] tiled against the reference, pose 3, 76 %
                                                 off (the six cases of (1, 4, 3) pass: pose 1 of its group is the
                                                 one nothing is accepted under, and bit 0 alone sorts the keys 0, 2
                                                 and all-ones that are left); mass fails every tiled case
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_reference as SR
from tests.test_parity_gpu import assert_close, grid_to_dev, tol
from tests.test_smooth_hard_gpu import (DTYPES, EDGE_GRIDS, INPUTS, M_FACTOR, N_BAD, N_FACE, TILE, budget_of, coords,
                                        far_cells_of, frozen, interior_cloud, r32, smooth_data, smooth_input,
                                        tile_count, to)

gpu = pytest.mark.gpu

PAIRS = [(2, 2), (3, 3), (3, 2)]
N_BORDER = 6  # the border points `smooth_input` puts in front
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")
VARIANTS = [("atomic", 0), ("tiled", 0), ("tiled", 1), ("tiled", 2)]  # algo, max_pose_group (2: groups of 2 + 1)
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "out"): 3.1127e-07,
    ("H3", "points"): 9.3890e-06,
    ("H3", "point_weight"): 9.1634e-06,
    ("H2_22", "out"): 7.7320e-07,
    ("H2_22", "points"): 8.5999e-06,
    ("H2_22", "point_weight"): 8.4952e-06,
    ("H2_32", "out"): 7.3559e-07,
    ("H2_32", "points"): 6.9781e-06,
    ("H2_32", "point_weight"): 6.6346e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def reference_out(c, dtype=np.float64):
    with np.errstate(invalid="ignore"):
        return np.stack([SR.raster_smooth(c.grid, c.points[b], c.rot[b:b + 1], c.trans[b:b + 1], c.bg[b:b + 1],
                                          c.ow[b:b + 1], c.pw[b], dtype=dtype)[..., 0] for b in range(c.B)], axis=-1)


def reference_pullback(c, dtype=np.float64):
    with np.errstate(invalid="ignore"):
        parts = [SR.raster_pullback_smooth(c.g[..., b:b + 1], c.points[b], c.rot[b:b + 1], c.trans[b:b + 1],
                                           c.ow[b:b + 1], c.pw[b], dtype=dtype) for b in range(c.B)]
    return (np.stack([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]),
            np.concatenate([p[4] for p in parts]), np.stack([p[5] for p in parts]))


def dev_args(c, tdt, dev, keep=slice(None)):
    t = lambda a: to(a, tdt, dev)
    return [t(c.points[:, keep]), t(c.rot), t(c.trans), t(c.bg), t(c.ow), t(c.pw[:, keep])]


def terms_of(c, b):
    """(accepted point indices, j0) of (cloud b, pose b)"""
    with np.errstate(invalid="ignore"):
        _b, idx, j0, _w, _dw = next(iter(SR._terms(c.grid, c.points[b], c.rot[b:b + 1], c.trans[b:b + 1], np.float64)))
    return idx, j0


def tile_of(grid, j0):
    """the tile of the clamped centre cell, axis 0 fastest (k_smooth_clouds_keys)"""
    nt = tile_count(grid)
    t = np.clip(j0, 0, np.asarray(grid) - 1) // np.asarray(TILE[len(grid)])
    return np.ravel_multi_index(tuple(t.T), nt, order="F") if len(j0) else np.zeros(0, np.int64)


# ------------------------------------------------------------------ 2a clustered clouds
@functools.lru_cache(maxsize=None)
def clustered(name):
    h, s = smooth_input(name), smooth_data(name)
    rng = np.random.default_rng(5100 + len(name) + h.n_in)
    head, body, tail = h.points[:N_BORDER], h.points[N_BORDER:-(N_FACE + N_BAD)], h.points[-(N_FACE + N_BAD):]
    clouds = [h.points, np.concatenate([head, body[::-1] * 0.9, tail]),
              np.concatenate([head, np.roll(body, 1000, axis=0) * 1.1, tail])]
    c = SimpleNamespace(name=name, n_in=h.n_in, n_out=h.n_out, grid=h.grid, P=h.P, B=3, points=r32(np.stack(clouds)),
                        rot=h.rot, trans=h.trans, bg=s.bg, ow=s.ow, pw=r32(rng.uniform(0.5, 1.5, size=(3, h.P))), g=s.g)
    frozen(c.points, c.pw)
    return c


@functools.lru_cache(maxsize=None)
def clustered_out(name, dtype=np.float64):
    out = reference_out(clustered(name), dtype)
    assert np.all(np.isfinite(out))
    return frozen(out)


@functools.lru_cache(maxsize=None)
def clustered_pullback(name, dtype=np.float64):
    pb = reference_pullback(clustered(name), dtype)
    assert all(np.all(np.isfinite(x)) for x in pb)
    frozen(*pb)
    return pb


@functools.lru_cache(maxsize=None)
def clustered_budget(name):
    c = clustered(name)
    E = np.stack([budget_of(c.grid, c.points[b], c.rot[b:b + 1], c.trans[b:b + 1], c.bg[b:b + 1], c.ow[b:b + 1],
                            c.pw[b])[..., 0] for b in range(c.B)], axis=-1)
    assert np.all(E > 0)
    return frozen(E)


@functools.lru_cache(maxsize=None)
def clustered_far(name):
    c = clustered(name)
    return frozen(np.stack([far_cells_of(c.grid, c.points[b], c.rot[b:b + 1], c.trans[b:b + 1])[..., 0]
                            for b in range(c.B)], axis=-1))


def measured_rho(name):
    r = {(name, "out"): float((np.abs(clustered_out(name, np.float32).astype(np.float64) - clustered_out(name))
                               / clustered_budget(name)).max())}
    p64, p32 = clustered_pullback(name), clustered_pullback(name, np.float32)
    for field, i in (("points", 0), ("point_weight", 5)):
        r[(name, field)] = float(np.abs(p32[i].astype(np.float64) - p64[i]).max() / np.abs(p64[i]).max())
    return r


@pytest.mark.parametrize("name", INPUTS)
def test_clustered_clouds_reach_the_regimes(name):
    """(CPU)  Every cloud under its own pose: a (pose, tile) run above 4 x 256 points (five rounds of the walk of
    k_smooth_clouds_tile), an empty tile in 3-D, rejected points, accepted points with j0 = -1 and with j0 = n_0."""
    c = clustered(name)
    tiles = int(np.prod(tile_count(c.grid)))
    for b in range(c.B):
        idx, j0 = terms_of(c, b)
        counts = np.bincount(tile_of(c.grid, j0), minlength=tiles)
        print(f"{name} cloud {b}: {tiles} tiles, heaviest {counts.max()}, empty {int((counts == 0).sum())}, "
              f"rejected {c.P - len(idx)}, j0 = -1: {int((j0[:, 0] == -1).sum())}, "
              f"j0 = n_0: {int((j0[:, 0] == c.grid[0]).sum())}")
        assert counts.max() > 4 * 256, (name, b)
        if c.n_out == 3:
            assert (counts == 0).any(), (name, b)
        assert c.P - len(idx) >= N_BAD + 1, (name, b)
        assert (j0[:, 0] == -1).any() and (j0[:, 0] == c.grid[0]).any(), (name, b)
        assert np.all(~np.isfinite(c.points[b, -N_BAD:]).all(axis=1)) and np.all(np.isfinite(c.points[b, :-N_BAD]))
    assert not np.array_equal(c.points[0], c.points[1]) and not np.array_equal(c.points[0], c.points[2])
    far, out = clustered_far(name), clustered_out(name)
    assert np.array_equal(out[far], np.broadcast_to(c.bg, out.shape)[far]) and far[..., 1].any() and far[..., 2].any()


@pytest.mark.parametrize("name", INPUTS)
def test_recorded_rho_is_the_reference_s(name):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 1 %."""
    for key, rho in measured_rho(name).items():
        print(f"rho {key}: {rho:.4e}")
        assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
        assert abs(RHO[key] - rho) <= 0.01 * rho, f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,group", VARIANTS)
@pytest.mark.parametrize("name", INPUTS)
def test_forward_cell_by_cell(dev, name, algo, group, npdt, tdt):
    c = clustered(name)
    ref64 = clustered_out(name)
    out = dpr_amd.raster_smooth_clouds(c.grid, *dev_args(c, tdt, dev), algo=algo, max_pose_group=group)
    assert tuple(out.shape) == c.grid + (c.B,) and out.dtype == tdt
    raw = out.cpu().numpy()
    got = raw.astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out"
    what = f"{name} {algo} group {group}"
    for b in range(c.B):
        assert_close(out[..., b], ref64[..., b].astype(npdt), tol(npdt, "out"), f"{what} plane {b}")
    if npdt == np.float32:
        E = clustered_budget(name)
        m = M_FACTOR * RHO[(name, "out")]
        ratio = np.abs(got - ref64) / E
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{what}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
        assert ratio.max() <= m, f"cell {worst}: |got - ref64| = {abs(got[worst] - ref64[worst]):.3e} > " \
            f"{m:.3e} * E = {m * E[worst]:.3e} ({int((ratio > m).sum())} cells over the bound)"
    far = clustered_far(name)
    bad = far & (raw != np.broadcast_to(c.bg.astype(npdt), raw.shape))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(far.sum())} far cells are not the background; " \
        f"first {tuple(int(v) for v in np.argwhere(bad)[0])}"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, npdt, tdt):
    c = clustered(name)
    ref = clustered_pullback(name)
    g = grid_to_dev(c.g.astype(npdt), dev)
    pb = dpr_amd.raster_pullback_smooth_clouds_(g, *dev_args(c, tdt, dev))
    for f, x in zip(FIELDS, pb):
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    for f, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        if kind == "pose" or npdt == np.float64:
            assert_close(a, e.astype(npdt), tol(npdt, kind), f"{name} {f}")
    faces = np.arange(c.P - N_BAD - N_FACE, c.P - N_BAD)
    for f, i in (("points", 0), ("point_weight", 5)):
        got, e = pb[i].cpu().numpy().astype(np.float64), ref[i]
        scale = np.abs(e).max()
        m = M_FACTOR * RHO[(name, f)] if npdt == np.float32 else tol(npdt, "points")
        d = np.abs(got - e).reshape(c.B, c.P, -1).max(axis=2)  # (cloud, point)
        print(f"{name} {np.dtype(npdt).name} ds_d{f}: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
              f"(m = {m:.3e}); face points {d[:, faces].max() / scale:.3e}")
        if npdt == np.float32:
            assert d.max() <= m * scale, f"ds_d{f}: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} at " \
                f"(cloud, point) {np.unravel_index(int(d.argmax()), d.shape)}"
        over = np.argwhere(d[:, faces] > m * scale)  # the cell-face points one by one
        assert len(over) == 0, f"ds_d{f} of face point {int(faces[over[0][1]])} of cloud {int(over[0][0])}: off by " \
            f"{d[over[0][0], faces[over[0][1]]]:.3e} > {m:.3e} * {scale:.3e}; {len(over)} face points over the bound"
    # the NaN / Inf rows are exactly 0; the point gradients are plain stores: the other rows do not know of the five
    assert not bool((pb.points[:, -N_BAD:] != 0).any()), "ds_dpoints of a NaN / Inf point is not 0"
    assert not bool((pb.point_weight[:, -N_BAD:] != 0).any()), "ds_dpoint_weight of a NaN / Inf point is not 0"
    keep = slice(0, c.P - N_BAD)
    pc = dpr_amd.raster_pullback_smooth_clouds_(g, *dev_args(c, tdt, dev, keep))
    assert torch.equal(pb.points[:, keep], pc.points), "ds_dpoints of the other points"
    assert torch.equal(pb.point_weight[:, keep], pc.point_weight), "ds_dpoint_weight of the other points"
    for f in ("rotation", "translation", "background", "out_weight"):
        assert_close(getattr(pb, f), getattr(pc, f).cpu().numpy(), tol(npdt, "pose"), f"ds_d{f} without the five")


# ------------------------------------------------------------------ 2b the key bits of a group
KEY_GRIDS = {1: {3: (5, 5, 5), 2: (5, 5)}, 3: {3: (48, 8, 8), 2: (192, 16)}, 4: {3: (32, 16, 8), 2: (65, 17)},
             7: {3: (112, 8, 8), 2: (448, 16)}}
# (tiles, B, max_pose_group): (nb * tiles, bits) of the full group, of the last group
KEY_CASES = {
    (1, 4, 3): ((3, 2), (1, 1)),
    (1, 5, 4): ((4, 3), (1, 1)),
    (1, 7, 5): ((5, 3), (2, 2)),
    (1, 8, 7): ((7, 3), (1, 1)),
    (1, 9, 8): ((8, 4), (1, 1)),
    (1, 16, 15): ((15, 4), (1, 1)),
    (1, 16, 16): ((16, 5), (16, 5)),
    (3, 2, 1): ((3, 2), (3, 2)),
    (3, 4, 3): ((9, 4), (3, 2)),
    (3, 7, 5): ((15, 4), (6, 3)),
    (4, 2, 1): ((4, 3), (4, 3)),
    (4, 3, 2): ((8, 4), (4, 3)),
    (4, 5, 4): ((16, 5), (4, 3)),
    (4, 5, 0): ((20, 5), (20, 5)),
    (7, 2, 1): ((7, 3), (7, 3)),
    (7, 3, 2): ((14, 4), (7, 3)),
    (7, 5, 0): ((35, 6), (35, 6)),
}
KEY_PARAMS = [(n_in, n_out, case) for case in KEY_CASES for n_in, n_out in PAIRS]


def key_bits(ge):
    """ord_key_bits of csrc/dpr_ordered_index.h"""
    bits = 1
    while bits < 32 and 2 ** bits - 1 < ge:
        bits += 1
    return bits


def group_of(B, max_group):
    """smooth_clouds_group for a small cloud (B * max(P, tiles) far below 2^24): B, cut to max_pose_group"""
    return min(B, max_group) if max_group > 0 else B


def empty_first_tile_pose(tiles, B, max_group):
    """the pose whose first tile is left empty: the second pose of the first group (None in groups of one; with one
    tile it holds no accepted point at all, so it must not be the last pose of its group)"""
    nb = group_of(B, max_group)
    return 1 if nb >= (3 if tiles == 1 else 2) else None


@functools.lru_cache(maxsize=None)
def key_case(n_in, n_out, case):
    from tests.test_smooth_clouds_gpu import _cloud, _poses
    tiles, B, max_group = case
    grid = KEY_GRIDS[tiles][n_out]
    rng = np.random.default_rng(5200 + 100 * n_in + 10 * n_out + sum(case))
    P = 500
    rot, trans = _poses(rng, B, n_in, n_out)
    n = np.asarray(grid, np.float64)
    hollow = empty_first_tile_pose(tiles, B, max_group)
    clouds = []
    for b in range(B):
        if b == hollow:  # nothing in the first tile: beyond it on axis 0, or (one tile) beyond the grid
            lo = n + 2.0 if tiles == 1 else np.asarray([TILE[n_out][0] + 0.5] + [-2.0] * (n_out - 1))
            pts = _cloud(rng, grid, rot[b], trans[b], n_in, P, lo=lo, hi=6.0 if tiles == 1 else 2.0)
        else:
            pts = _cloud(rng, grid, rot[b], trans[b], n_in, P)
        if not (b == hollow and tiles == 1):  # an accepted point in the last cell, so in the last tile
            pts[0] = ((-1 + 2 * (n - 0.5) / n) - trans[b]) @ rot[b]
        clouds.append(pts)
    c = SimpleNamespace(n_in=n_in, n_out=n_out, grid=grid, P=P, B=B, tiles=tiles, max_group=max_group, hollow=hollow,
                        points=r32(np.stack(clouds)), rot=r32(rot), trans=r32(trans), bg=r32(rng.normal(size=B)),
                        ow=r32(rng.uniform(0.5, 1.5, size=B)), pw=r32(rng.uniform(0.5, 1.5, size=(B, P))))
    c.out = reference_out(c)
    assert np.all(np.isfinite(c.out))
    frozen(c.points, c.rot, c.trans, c.bg, c.ow, c.pw, c.out)
    return c


def test_key_cases_cover_the_key_bit_edges():
    """(CPU)  nb * tiles of the full group takes 2^k - 1, 2^k and 2^k + 1; a last group with other bits than the
    full one occurs more than once; KEY_CASES lists what the launch computes."""
    full, differ = set(), 0
    for (tiles, B, max_group), want in KEY_CASES.items():
        assert all(int(np.prod(tile_count(g))) == tiles == EDGE_GRIDS[g] for g in KEY_GRIDS[tiles].values())
        nb = group_of(B, max_group)
        last = B % nb or nb
        got = ((nb * tiles, key_bits(nb * tiles)), (last * tiles, key_bits(last * tiles)))
        print(f"tiles {tiles}, B {B}, max_pose_group {max_group}: full group {got[0]}, last group {got[1]}")
        assert got == want
        for ge, bits in got:  # the all-ones key of a rejected point, cut to `bits` bits, sorts behind the last tile
            assert 2 ** bits - 1 >= ge and (bits == 1 or 2 ** (bits - 1) - 1 < ge)
        full.add(nb * tiles)
        differ += got[0][1] != got[1][1]
    assert {3, 4, 5, 7, 8, 9, 15, 16} <= full, full
    assert differ >= 2


@pytest.mark.parametrize("n_in,n_out,case", KEY_PARAMS)
def test_key_clouds_are_what_the_cases_need(n_in, n_out, case):
    """(CPU)  Every pose has rejected points (the run of the all-ones keys is never empty); the last tile of the last
    pose of every group holds an accepted point (its run touches that run); one non-first pose of a group has an
    empty first tile (a start-table entry shared with the pose before it)."""
    c = key_case(n_in, n_out, case)
    nb = group_of(c.B, c.max_group)
    for b in range(c.B):
        idx, j0 = terms_of(c, b)
        tile = tile_of(c.grid, j0)
        assert len(idx) < c.P, f"pose {b}: no rejected point"
        if b % nb == nb - 1 or b == c.B - 1:
            assert (tile == c.tiles - 1).any(), f"pose {b}, the last of its group: nothing in the last tile"
        if b == c.hollow:
            assert 0 < b % nb and not (tile == 0).any() and (c.tiles == 1 or len(idx) > 0)
        else:
            assert len(idx) > 0
    assert (c.hollow is not None) == (nb >= (3 if c.tiles == 1 else 2))


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,case", KEY_PARAMS)
def test_key_bits_of_a_group(dev, n_in, n_out, case, npdt, tdt):
    c = key_case(n_in, n_out, case)
    args = dev_args(c, tdt, dev)
    need = dpr_amd.workspace_bytes_smooth_clouds("raster", c.grid, c.P, c.B, n_in, tdt, "tiled",
                                                 max_pose_group=c.max_group)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tiled = dpr_amd.raster_smooth_clouds(c.grid, *args, algo="tiled", max_pose_group=c.max_group, workspace=ws)
    atomic = dpr_amd.raster_smooth_clouds(c.grid, *args, algo="atomic")
    assert bool(torch.isfinite(tiled).all()) and bool(torch.isfinite(atomic).all())
    for b in range(c.B):  # plane by plane: a pose must not hide in the others' norm
        e = c.out[..., b].astype(npdt)
        assert_close(tiled[..., b], e, tol(npdt, "out"), f"{case} tiled, pose {b}")
        assert_close(atomic[..., b], e, tol(npdt, "out"), f"{case} atomic, pose {b}")
        assert_close(tiled[..., b], atomic[..., b].cpu().numpy(), tol(npdt, "out"), f"{case} tiled vs atomic, pose {b}")
    if c.hollow is not None and c.tiles == 1:  # a pose nothing is accepted under: exactly its background
        assert bool((tiled[..., c.hollow] == float(c.bg[c.hollow].astype(npdt))).all())


# ------------------------------------------------------------------ 2c mass
@functools.lru_cache(maxsize=None)
def interior_clouds(n_in, n_out):
    """`interior_cloud` as three clouds: cloud b is its rows rolled by 1 000 b and scaled, as interior_cloud scales,
    to stay at least 2 cells inside the grid under pose b alone."""
    c = interior_cloud(n_in, n_out)
    clouds = []
    for b in range(c.B):
        pts = np.roll(c.points, 1000 * b, axis=0)
        room = 1.0 - 4.0 / np.asarray(c.grid, np.float64) - np.abs(c.trans[b])
        reach = np.abs(pts @ c.rot[b].T).max(axis=0)
        clouds.append(pts * (0.999 * (room / reach).min()))
    m = SimpleNamespace(grid=c.grid, B=c.B, P=c.P, points=r32(np.stack(clouds)), rot=c.rot, trans=c.trans, bg=c.bg,
                        ow=c.ow, pw=r32(np.stack([np.roll(c.pw, 77 * b) * (1 + 0.25 * b) for b in range(c.B)])))
    frozen(m.points, m.pw)
    return m


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_interior_clouds_are_interior(n_in, n_out):
    m = interior_clouds(n_in, n_out)
    for b in range(m.B):
        co = coords(m.grid, m.points[b], m.rot[b], m.trans[b])
        assert co.min() >= 2 and np.all(co <= np.asarray(m.grid) - 2), (b, co.min(axis=0), co.max(axis=0))
        assert np.ptp(co, axis=0).min() > 0.25 * min(m.grid)
    assert not np.array_equal(m.points[0], m.points[1])


@gpu
@pytest.mark.parametrize("algo,group", VARIANTS)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_mass_of_interior_clouds(dev, n_in, n_out, algo, group):
    """fp64: |sum out[.., b] - G bg_b - ow_b sum pw_b| <= (3^N P + G) eps (G |bg_b| + |ow_b| sum |pw_b|), the
    any-order worst case for that many additions; the plane is summed on the device in fp64."""
    m = interior_clouds(n_in, n_out)
    out = dpr_amd.raster_smooth_clouds(m.grid, *dev_args(m, torch.float64, dev), algo=algo, max_pose_group=group)
    total = out.sum(dim=tuple(range(n_out))).cpu().numpy()
    G = int(np.prod(m.grid))
    eps = float(np.finfo(np.float64).eps)
    for b in range(m.B):
        want = G * m.bg[b] + m.ow[b] * m.pw[b].sum()
        bound = (3 ** n_out * m.P + G) * eps * (G * abs(m.bg[b]) + abs(m.ow[b]) * np.abs(m.pw[b]).sum())
        print(f"({n_in}, {n_out}) {algo} group {group} pose {b}: mass off by {abs(total[b] - want):.3e}, "
              f"bound {bound:.3e}")
        assert abs(total[b] - want) <= bound, (b, total[b], want, bound)
