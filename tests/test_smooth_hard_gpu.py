"""The smooth splat (csrc/dpr_smooth.hip) in the regimes the other op families are held to: clustered clouds with
cell-face and NaN / Inf points, a bound per cell in fp32, cells nothing reaches, mass, the key-bit and small-grid
edges of the tiled forward, the pose-inside-thread pullback of a batch, and raster_smooth_ad beyond fp64 / default.

Every expectation is tests/smooth_reference.py (`SR`) in fp64 on inputs rounded to fp32 once and used for both
dtypes.  The hard inputs are hard("H3"), hard("H2_22") and hard("H2_32") of tests/test_families_hard_gpu.py with
fp32-rounded point_weight and out_weight in [0.5, 1.5], a non-zero background and ds_dout ~ N(0, 1) added
(`smooth_data`).  On the smooth tiles (SmoothTileShape in csrc/dpr_smooth.h: 3-D 16 x 8 x 8, 2-D 64 x 16), counted on
the CPU from the reference's cell choice (test_hard_inputs_reach_the_regimes recounts and asserts the regimes):

    input   tiles              heaviest tile (pose 0 / 1 / 2)    empty tiles       rejected points
    H3      9 x 9 x 5 = 405    88 317 / 90 320 / 116 592         108 / 111 / 134   65 / 102 / 133
    H2_22   2 x 5 = 10         37 937 / 25 945 / 30 496          0 / 0 / 0         22 / 35 / 45
    H2_32   2 x 5 = 10         38 095 / 33 709 / 20 863          0 / 0 / 0         21 / 39 / 50

(`smooth_input` puts six border points in front of each cloud, so that every pose has an accepted point whose centre
cell is -1 and one whose centre cell is n_0; without them the counts are hard()'s own, H3: 110 / 112 / 136 empty
tiles, 65 / 102 / 132 rejected points.)

The fp32 bound per cell (A.1).  For every cell c and pose b the budget, formed in fp64 from SR._terms,

    E[c, b] = |background[b]| + sum_p |ow_b pw_p| ( prod_d w_d + sum_k |coord_k| |w'_k| prod_{d != k} w_d )

over the contributions that land on c: the contribution itself plus its first-order sensitivity to a relative
perturbation of coord (a weight near 0 has unbounded relative error under coordinate rounding).  The assertion is
|got - ref64| <= m E on EVERY cell, m = M_FACTOR * rho_cell, rho_cell = max over cells and poses of
|ref32 - ref64| / E with ref32 = SR.raster_smooth(dtype = fp32): the reference's own fp32 rounding, measured on the
CPU, never on the device (test_recorded_rho_is_the_reference_s re-measures it).  The pullback's ds_dpoints and
ds_dpoint_weight (A.5) follow test_families_hard_gpu.py's convention, max|got - ref64| <= 4 rho max|ref64| with
rho = max|ref32 - ref64| / max|ref64| of the fp32 reference, per batch size.

    rho, CPU reference    forward, per cell    ds_dpoints B=1 / B=3       ds_dpoint_weight B=1 / B=3
    H3                    9.168e-07            1.216e-05 / 1.018e-05      8.542e-06 / 6.334e-06
    H2_22                 5.259e-07            7.966e-06 / 6.744e-06      8.188e-06 / 6.351e-06
    H2_32                 7.052e-07            5.780e-06 / 5.681e-06      7.380e-06 / 4.953e-06

Observed on an MI355X (the tests print them; with B = 3 the atomics' arrival order moves the last digits):

    forward, fp32: max |got - ref64| / E    m           atomic B=1 / B=3         tiled B=1 / B=3
    H3                                      3.667e-06   1.07e-07 / 9.46e-07      9.83e-08 / 9.46e-07
    H2_22                                   2.103e-06   8.67e-08 / 8.32e-07      8.67e-08 / 8.32e-07
    H2_32                                   2.821e-06   9.05e-08 / 7.05e-07      9.05e-08 / 7.05e-07
    (B = 3: one cell of pose 1 or 2 whose nearest point changes its centre cell between fp32 and fp64 coordinates
    -- the reference's own worst cell; everywhere else, and with the identity pose alone, a tenth of it.)

    pullback, fp32: max |got - ref64| / max |ref64| (m)    ds_dpoints B=1 / B=3                   ds_dpoint_weight B=1 / B=3
    H3      1.21e-05 (4.86e-05) / 1.07e-05 (4.07e-05)      8.57e-06 (3.42e-05) / 7.05e-06 (2.53e-05)
    H2_22   7.87e-06 (3.19e-05) / 9.21e-06 (2.70e-05)      8.22e-06 (3.28e-05) / 1.01e-05 (2.54e-05)
    H2_32   5.80e-06 (2.31e-05) / 8.09e-06 (2.27e-05)      7.40e-06 (2.95e-05) / 5.69e-06 (1.98e-05)
    the 64 cell-face points alone: at most 4.7e-06; fp64: at most 1.4e-14 everywhere.

    mass, fp64: off by at most 3.7e-12 (one ulp of the sum) against bounds of 5.4e-07 .. 4.7e-06.

The mass bound (A.3) is derived, not measured: the any-order worst case of (3^N P + G) additions.

Mutation record (scratch builds of libdpr, one MI355X run each; every mutant keeps its accesses inside the buffers:
a dropped contribution writes nothing, a kept fetch reads cell 0 of its pose).  Each line: the mutant, the first
test and assertion that failed.  (The offset and stride mutants: tests/test_index_ranges_gpu.py.)
  k_smooth_tile `l < e[d] + 2` -> `+ 1`        forward_cell_by_cell[H3-tiled-1-float32]: the norm-wise comparison,
  (the high halo cell dropped)                 7 % off (atomic passes before); mass[2-2-tiled]: pose 0, 138 of 20 185
  smooth_fwd_tiled sorts on bits - 1 bits      key_bit_and_small_grid_edges[(32, 8, 8)-float64]: tiled against the
                                               reference, 81 % off (the twelve one-tile cases before it pass)
  k_smooth_bwd keeps the value fetched from    pullback_element_by_element[H3-1-float64]: ds_dpoints, 5.4e-3 off
  cell 0 for a dropped cell (no select)        (fp64 runs first; the face-point rows were not reached)
  pose_slices forced to two slices at          pullback_of_a_batch_at_the_slice_threshold (B = 3): SURVIVED, all eight
  P = 524 033                                  cases pass -- slices of 2 + 1 poses add (p0 + p1) + p2 onto zero as well.
                                               test_one_slice_adds_four_poses_in_index_order was added for it: two
                                               slices of 2 + 2 poses add (p0 + p1) + (p2 + p3), which that test asserts
                                               to differ from ((p0 + p1) + p2) + p3 on its input (argued, not run)
Argued, not run: a mutant that widens the LDS window (`l < e[d] + 3`) or drops the `c < gd.n[d]` test writes past
the LDS array or the plane.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_reference as SR
from tests.test_families_hard_gpu import M_FACTOR, hard, r32
from tests.test_parity_gpu import assert_close, grid_to_dev, tol

gpu = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
INPUTS = ("H3", "H2_22", "H2_32")
# SmoothTileShape of csrc/dpr_smooth.h
TILE = {3: (16, 8, 8), 2: (64, 16)}
N_BAD, N_FACE = 5, 64  # the tail of a hard cloud: 64 cell-face points, then 5 NaN / Inf points
SEED = {"H3": 3001, "H2_22": 3002, "H2_32": 3003}
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "out"): 9.1684e-07,
    ("H3", "points", 1): 1.2160e-05,
    ("H3", "point_weight", 1): 8.5421e-06,
    ("H3", "points", 3): 1.0175e-05,
    ("H3", "point_weight", 3): 6.3342e-06,
    ("H2_22", "out"): 5.2586e-07,
    ("H2_22", "points", 1): 7.9664e-06,
    ("H2_22", "point_weight", 1): 8.1876e-06,
    ("H2_22", "points", 3): 6.7439e-06,
    ("H2_22", "point_weight", 3): 6.3507e-06,
    ("H2_32", "out"): 7.0523e-07,
    ("H2_32", "points", 1): 5.7803e-06,
    ("H2_32", "point_weight", 1): 7.3802e-06,
    ("H2_32", "points", 3): 5.6812e-06,
    ("H2_32", "point_weight", 3): 4.9533e-06,
}
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KINDS = ("points", "pose", "pose", "pose", "pose", "points")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def to(a, tdt, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev).to(tdt)  # (a copy: the cached inputs are read-only)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def tile_count(grid):
    return tuple(-(-n // e) for n, e in zip(grid, TILE[len(grid)]))


# ------------------------------------------------------------------ the inputs and their references (computed once)
@functools.lru_cache(maxsize=None)
def smooth_input(name):
    """hard(name) with six border points in front: for every pose one point at coord_0 = -1/2 (centre cell
    j0 = -1) and one at coord_0 = n_0 + 1/2 (j0 = n_0), at the middle of the other axes.  hard("H2_32") alone has no
    accepted point with j0 = -1 under pose 1.  The tail (face points, NaN / Inf points) stays the tail."""
    base = hard(name)
    border = []
    for b in range(base.B):
        for x0 in (-1.0 - 1.0 / base.grid[0], 1.0 + 1.0 / base.grid[0]):
            x = np.zeros(base.n_out)
            x[0] = x0
            border.append(np.linalg.pinv(base.rot[b]) @ (x - base.trans[b]))
    pts = frozen(r32(np.concatenate([np.asarray(border), base.points])))
    return SimpleNamespace(name=name, n_in=base.n_in, n_out=base.n_out, grid=base.grid, P=len(pts), B=base.B,
                           points=pts, rot=base.rot, trans=base.trans)


@functools.lru_cache(maxsize=None)
def smooth_data(name):
    h = smooth_input(name)
    rng = np.random.default_rng(SEED[name])
    bg = r32(rng.normal(size=h.B))
    bg[np.abs(bg) < 0.05] = 0.05
    s = SimpleNamespace(pw=r32(rng.uniform(0.5, 1.5, size=h.P)), ow=r32(rng.uniform(0.5, 1.5, size=h.B)), bg=r32(bg),
                        g=r32(rng.normal(size=h.grid + (h.B,))))
    assert np.all(s.bg != 0)
    frozen(s.pw, s.ow, s.bg, s.g)
    return s


@functools.lru_cache(maxsize=None)
def reference_out(name, dtype=np.float64):
    h, s = smooth_input(name), smooth_data(name)
    with np.errstate(invalid="ignore"):
        out = SR.raster_smooth(h.grid, h.points, h.rot, h.trans, s.bg, s.ow, s.pw, dtype=dtype)
    assert np.all(np.isfinite(out))
    return frozen(out)


@functools.lru_cache(maxsize=None)
def reference_pullback(name, B, dtype=np.float64):
    h, s = smooth_input(name), smooth_data(name)
    with np.errstate(invalid="ignore"):
        pb = SR.raster_pullback_smooth(s.g[..., :B], h.points, h.rot[:B], h.trans[:B], s.ow[:B], s.pw, dtype=dtype)
    assert all(np.all(np.isfinite(x)) for x in pb)
    frozen(*pb)
    return pb


def coords(grid, points, R, t):
    """coord of SR._terms in fp64, every point (NaN / Inf rows stay non-finite)"""
    n = np.asarray(grid, np.float64)
    with np.errstate(invalid="ignore"):
        return ((points @ R.T + t) + 1.0) * (n / 2.0)


def budget_of(grid, points, rot, trans, bg, ow, pw):
    """E[c, b] of the module docstring for any cloud, grid + (B,), fp64 (the core of `budget`; the hard tests of the
    other smooth families form it with a channel's or a cloud's own weights)."""
    N, B = len(grid), len(rot)
    E = np.empty(tuple(grid) + (B,))
    with np.errstate(invalid="ignore"):
        terms = list(SR._terms(grid, points, rot, trans, np.float64))
    for b, idx, j0, w, dw in terms:
        c = np.abs(coords(grid, points, rot[b], trans[b])[idx])
        plane = np.full(grid, abs(bg[b]))
        scale = np.abs(ow[b] * pw[idx])
        for st in itertools.product(range(3), repeat=N):
            cell = j0 + (np.asarray(st) - 1)
            inside = np.all((cell >= 0) & (cell < np.asarray(grid)), axis=1)
            v = np.ones(len(idx))
            for d in range(N):
                v = v * w[:, d, st[d]]
            for k in range(N):
                sens = c[:, k] * np.abs(dw[:, k, st[k]])
                for d in range(N):
                    if d != k:
                        sens = sens * w[:, d, st[d]]
                v = v + sens
            np.add.at(plane, tuple(cell[inside].T), (scale * v)[inside])
        E[..., b] = plane
    return E


@functools.lru_cache(maxsize=None)
def budget(name):
    """E[c, b] of the module docstring, grid + (B,), fp64."""
    h, s = smooth_input(name), smooth_data(name)
    E = budget_of(h.grid, h.points, h.rot, h.trans, s.bg, s.ow, s.pw)
    assert np.all(E > 0)
    return frozen(E)


def measured_rho(name):
    """{key: rho} of the CPU reference, the keys of RHO."""
    r = {(name, "out"): float((np.abs(reference_out(name, np.float32).astype(np.float64) - reference_out(name))
                               / budget(name)).max())}
    for B in (1, 3):
        p64, p32 = reference_pullback(name, B), reference_pullback(name, B, np.float32)
        for field, i in (("points", 0), ("point_weight", 5)):
            r[(name, field, B)] = float(np.abs(p32[i].astype(np.float64) - p64[i]).max() / np.abs(p64[i]).max())
    return r


def far_cells_of(grid, points, rot, trans):
    """grid + (B,) bool: no point of the pose has |coord_d - (c_d + 1/2)| < 2 on every axis (the true reach is 1.5
    cells; the extra half cell is far above any coordinate rounding).  The core of `far_cells`, for any cloud."""
    n = np.asarray(grid)
    far = np.ones(tuple(grid) + (len(rot),), bool)
    for b in range(len(rot)):
        c = coords(grid, points, rot[b], trans[b])
        c = c[np.all(np.isfinite(c) & (np.abs(c) < 1e6), axis=1)]
        lo = np.floor(c - 2.5).astype(np.int64) + 1  # the cells with c_d + 1/2 in (coord_d - 2, coord_d + 2)
        hi = np.ceil(c + 1.5).astype(np.int64) - 1
        assert (hi - lo).max() <= 4
        near = np.zeros(grid, bool)
        for k in itertools.product(range(5), repeat=len(grid)):
            cell = lo + np.asarray(k)
            okay = np.all((cell <= hi) & (cell >= 0) & (cell < n), axis=1)
            near[tuple(cell[okay].T)] = True
        far[..., b] = ~near
    return far


@functools.lru_cache(maxsize=None)
def far_cells(name):
    h = smooth_input(name)
    return frozen(far_cells_of(h.grid, h.points, h.rot, h.trans))


def dev_args(h, s, tdt, dev, B, keep=slice(None)):
    t = lambda a: to(a, tdt, dev)
    return [t(h.points[keep]), t(h.rot[:B]), t(h.trans[:B]), t(s.bg[:B]), t(s.ow[:B]), t(s.pw[keep])]


def check_pullback(pb, ref, npdt, what=""):
    for name, kind, a, e in zip(FIELDS, KINDS, pb, ref):
        assert_close(a, np.asarray(e).astype(npdt), tol(npdt, kind), f"{what}{name}")


# ------------------------------------------------------------------ A.0 the regime is what the table says (CPU)
@pytest.mark.parametrize("name", INPUTS)
def test_hard_inputs_reach_the_regimes(name):
    """Recounted from the reference's cell choice, per pose: a tile above 256 points (more than one round of the
    workgroup), an empty tile (H3), rejected points, and accepted points whose centre cell lies outside the grid on
    either side (j0 = -1 and j0 = n_d).  A change of the generator cannot drop a regime silently."""
    h = smooth_input(name)
    nt = tile_count(h.grid)
    assert nt == {"H3": (9, 9, 5)}.get(name, (2, 5))
    assert all(n % e != 0 for n, e in zip(h.grid, TILE[h.n_out])), "a tile remainder on every axis"
    n = np.asarray(h.grid)
    with np.errstate(invalid="ignore"):
        terms = list(SR._terms(h.grid, h.points, h.rot, h.trans, np.float64))
    for b, idx, j0, _w, _dw in terms:
        counts = np.zeros(nt, np.int64)
        np.add.at(counts, tuple((np.clip(j0, 0, n - 1) // np.asarray(TILE[h.n_out])).T), 1)
        rejected = h.P - len(idx)
        print(f"{name} pose {b}: {counts.size} tiles, heaviest {counts.max()}, empty {int((counts == 0).sum())}, "
              f"rejected {rejected}, j0 = -1: {int((j0 == -1).any(axis=1).sum())}, "
              f"j0 = n: {int((j0 == n).any(axis=1).sum())}")
        assert counts.max() > 256, (name, b)
        if name == "H3":
            assert (counts == 0).any(), (name, b)
        assert rejected >= N_BAD + 1, (name, b, rejected)
        assert (j0 == -1).any() and (j0 == n).any(), (name, b)
    # the tail of the cloud is what the tests below take it for
    assert np.all(~np.isfinite(h.points[-N_BAD:]).all(axis=1)) and np.all(np.isfinite(h.points[:-N_BAD]))


@pytest.mark.parametrize("name", INPUTS)
def test_recorded_rho_is_the_reference_s(name):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 1 %."""
    for key, rho in measured_rho(name).items():
        print(f"rho {key}: {rho:.4e}")
        assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
        assert abs(RHO[key] - rho) <= 0.01 * rho, f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@pytest.mark.parametrize("name", INPUTS)
def test_far_cells_hold_the_background_in_the_reference(name):
    """(CPU)  `far_cells` marks no cell a point reaches: there the fp64 reference is the background exactly."""
    far, out, s = far_cells(name), reference_out(name), smooth_data(name)
    assert np.array_equal(out[far], np.broadcast_to(s.bg, out.shape)[far])
    assert not np.array_equal(out, np.broadcast_to(s.bg, out.shape))


# ------------------------------------------------------------------ A.1 the forward, cell by cell
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("name", INPUTS)
def test_forward_cell_by_cell(dev, name, algo, B, npdt, tdt):
    h, s = smooth_input(name), smooth_data(name)
    ref64 = reference_out(name)[..., :B]
    out = dpr_amd.raster_smooth(h.grid, *dev_args(h, s, tdt, dev, B), algo=algo)
    assert tuple(out.shape) == h.grid + (B,) and out.dtype == tdt
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out"
    assert_close(out, ref64.astype(npdt), tol(npdt, "out"), f"{name} {algo} B={B}")
    if npdt == np.float32:
        E = budget(name)[..., :B]
        m = M_FACTOR * RHO[(name, "out")]
        ratio = np.abs(got - ref64) / E
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{name} {algo} B={B}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
        assert ratio.max() <= m, f"cell {worst}: |got - ref64| = {abs(got[worst] - ref64[worst]):.3e} > " \
            f"{m:.3e} * E = {m * E[worst]:.3e} ({int((ratio > m).sum())} cells over the bound)"


# ------------------------------------------------------------------ A.2 cells nothing reaches
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("name", INPUTS)
def test_cells_nothing_reaches_hold_the_background(dev, name, algo, npdt, tdt):
    h, s = smooth_input(name), smooth_data(name)
    far = far_cells(name)
    for b in range(h.B):
        assert far[..., b].any(), f"{name} pose {b}: no far cell"
    if name == "H3":
        assert far.sum() > 700_000  # (of 3 x 336 700 cells)
    out = dpr_amd.raster_smooth(h.grid, *dev_args(h, s, tdt, dev, h.B), algo=algo).cpu().numpy()
    want = np.broadcast_to(s.bg.astype(npdt), out.shape)
    bad = far & (out != want)
    assert not bad.any(), f"{name} {algo}: {int(bad.sum())} of {int(far.sum())} far cells are not the background; " \
        f"first {tuple(int(v) for v in np.argwhere(bad)[0])}"


# ------------------------------------------------------------------ A.3 mass
@functools.lru_cache(maxsize=None)
def interior_cloud(n_in, n_out):
    """20 000 points whose coordinates stay at least 2 cells inside the grid under each of 3 poses: a uniform cloud,
    scaled.  Nothing is dropped or rejected, so every point deposits exactly out_weight * point_weight."""
    from tests.test_smooth_gpu import GRIDS, _poses
    rng = np.random.default_rng(7000 + 10 * n_in + n_out)
    grid, B, P = GRIDS[n_out], 3, 20_000
    rot, trans = (r32(a) for a in _poses(rng, B, n_in, n_out))
    pts = rng.uniform(-1, 1, size=(P, n_in))
    room = 1.0 - 4.0 / np.asarray(grid, np.float64) - np.abs(trans).max(axis=0)
    reach = np.abs(np.einsum("bok,pk->bpo", rot, pts)).max(axis=(0, 1))
    pts = r32(pts * (0.999 * (room / reach).min()))
    c = SimpleNamespace(grid=grid, B=B, P=P, points=pts, rot=rot, trans=trans, bg=r32(rng.normal(size=B)),
                        ow=r32(rng.uniform(0.5, 1.5, size=B)), pw=r32(rng.uniform(0.5, 1.5, size=P)))
    frozen(c.points, c.rot, c.trans, c.bg, c.ow, c.pw)
    return c


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_interior_cloud_is_interior(n_in, n_out):
    c = interior_cloud(n_in, n_out)
    assert c.grid in ((37, 19, 21), (150, 37)) and all(n % e != 0 for n, e in zip(c.grid, TILE[n_out]))
    for b in range(c.B):
        co = coords(c.grid, c.points, c.rot[b], c.trans[b])
        assert co.min() >= 2 and np.all(co <= np.asarray(c.grid) - 2), (b, co.min(axis=0), co.max(axis=0))
    assert np.ptp(co, axis=0).min() > 0.25 * min(c.grid)  # (still a cloud over many cells and several tiles)


@gpu
@pytest.mark.parametrize("algo", ["atomic", "tiled"])
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_mass_of_an_interior_cloud(dev, n_in, n_out, algo):
    """fp64: |sum out[.., b] - G bg_b - ow_b sum pw| <= (3^N P + G) eps (G |bg_b| + |ow_b| sum |pw|), the any-order
    worst case for that many additions; the plane is summed on the device in fp64."""
    c = interior_cloud(n_in, n_out)
    t = lambda a: to(a, torch.float64, dev)
    out = dpr_amd.raster_smooth(c.grid, t(c.points), t(c.rot), t(c.trans), t(c.bg), t(c.ow), t(c.pw), algo=algo)
    total = out.sum(dim=tuple(range(n_out))).cpu().numpy()
    G = int(np.prod(c.grid))
    eps = float(np.finfo(np.float64).eps)
    for b in range(c.B):
        want = G * c.bg[b] + c.ow[b] * c.pw.sum()
        bound = (3 ** n_out * c.P + G) * eps * (G * abs(c.bg[b]) + abs(c.ow[b]) * np.abs(c.pw).sum())
        print(f"({n_in}, {n_out}) {algo} pose {b}: mass off by {abs(total[b] - want):.3e}, bound {bound:.3e}")
        assert abs(total[b] - want) <= bound, (b, total[b], want, bound)


# ------------------------------------------------------------------ A.4 NaN / Inf points
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("name", INPUTS)
def test_nan_and_inf_points_poison_nothing(dev, name, npdt, tdt):
    h, s = smooth_input(name), smooth_data(name)
    keep = slice(0, h.P - N_BAD)
    for B in (1, 3):
        g = grid_to_dev(s.g[..., :B].astype(npdt), dev)
        full, clean = dev_args(h, s, tdt, dev, B), dev_args(h, s, tdt, dev, B, keep)
        pb = dpr_amd.raster_pullback_smooth_(g, *full)
        pc = dpr_amd.raster_pullback_smooth_(g, *clean)
        for f, x in zip(FIELDS, pb):
            assert bool(torch.isfinite(x).all()), f"B={B}: non-finite ds_d{f}"
        assert not bool((pb.points[-N_BAD:] != 0).any()), f"B={B}: ds_dpoints of a NaN / Inf point is not 0"
        assert not bool((pb.point_weight[-N_BAD:] != 0).any()), f"B={B}: ds_dpoint_weight of a NaN / Inf point"
        if B == 1:  # one thread per point, plain store: the other rows do not know of the five
            assert torch.equal(pb.points[keep], pc.points), "ds_dpoints of the other points"
            assert torch.equal(pb.point_weight[keep], pc.point_weight), "ds_dpoint_weight of the other points"
        else:
            assert_close(pb.points[keep], pc.points.cpu().numpy(), tol(npdt, "points"), "ds_dpoints")
            assert_close(pb.point_weight[keep], pc.point_weight.cpu().numpy(), tol(npdt, "points"),
                         "ds_dpoint_weight")
        for f in ("rotation", "translation", "background", "out_weight"):
            assert_close(getattr(pb, f), getattr(pc, f).cpu().numpy(), tol(npdt, "pose"), f"B={B}: ds_d{f}")
        for algo in ("atomic", "tiled"):
            a = dpr_amd.raster_smooth(h.grid, *full, algo=algo)
            b = dpr_amd.raster_smooth(h.grid, *clean, algo=algo)
            assert bool(torch.isfinite(a).all()), f"B={B} {algo}: non-finite out"
            assert_close(a, b.cpu().numpy(), tol(npdt, "out"), f"B={B} {algo}: out with and without the five")


# ------------------------------------------------------------------ A.5 the pullback, element by element
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, B, npdt, tdt):
    h, s = smooth_input(name), smooth_data(name)
    ref = reference_pullback(name, B)
    pb = dpr_amd.raster_pullback_smooth_(grid_to_dev(s.g[..., :B].astype(npdt), dev), *dev_args(h, s, tdt, dev, B))
    for f, x in zip(FIELDS, pb):
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    if npdt == np.float64:
        check_pullback(pb, ref, npdt, f"{name} B={B} ")
    else:
        for f, kind, a, e in zip(FIELDS, KINDS, pb, ref):
            if kind == "pose":
                assert_close(a, e.astype(npdt), tol(npdt, "pose"), f"{name} B={B} {f}")
    faces = np.arange(h.P - N_BAD - N_FACE, h.P - N_BAD)
    for f, i in (("points", 0), ("point_weight", 5)):
        got, e = pb[i].cpu().numpy().astype(np.float64), ref[i]
        scale = np.abs(e).max()
        m = M_FACTOR * RHO[(name, f, B)] if npdt == np.float32 else tol(npdt, "points")
        d = np.abs(got - e)
        print(f"{name} B={B} {np.dtype(npdt).name} ds_d{f}: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
              f"(m = {m:.3e}); face points {d[faces].max() / scale:.3e}")
        if npdt == np.float32:
            assert d.max() <= m * scale, f"ds_d{f}: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} at " \
                f"point {int(np.argmax(d.reshape(h.P, -1).max(axis=1)))}"
        # the cell-face points one by one
        row = d.reshape(h.P, -1).max(axis=1)[faces]
        over = np.nonzero(row > m * scale)[0]
        assert len(over) == 0, f"ds_d{f} of face point {int(faces[over[0]])} ({h.points[faces[over[0]]]}): off by " \
            f"{row[over[0]]:.3e} > {m:.3e} * {scale:.3e}; {len(over)} face points over the bound"


# ------------------------------------------------------------------ A.6 key bits and small grids
EDGE_GRIDS = {  # grid: tiles
    (5, 5, 5): 1, (16, 8, 8): 1, (5, 5): 1, (64, 16): 1,
    (32, 8, 8): 2, (128, 16): 2,
    (48, 8, 8): 3, (192, 16): 3,
    (32, 16, 8): 4, (65, 17): 4,
    (112, 8, 8): 7, (448, 16): 7,
    (32, 16, 16): 8, (17, 9, 9): 8, (128, 64): 8,
    # thin axes
    (1, 1, 1): 1, (2, 1, 3): 1, (1, 1): 1, (1, 40): 3, (2, 2): 1,
}
EDGE_CASES = [(n_in, len(grid), grid) for grid in EDGE_GRIDS for n_in in ((3,) if len(grid) == 3 else (2, 3))]


@functools.lru_cache(maxsize=None)
def edge_case(n_in, grid):
    """3000 points uniform in +-1.3, one point at the centre of every corner cell (and one that the second pose puts
    at the centre of the last cell: the last tile of (65, 17) is that one cell), and six points no pose accepts
    (two with NaN / Inf coordinates, four far outside: the uniform part alone has no rejected point on an axis of
    fewer than 7 cells under the identity).  B = 2: the identity and one random pose."""
    from tests.test_smooth_gpu import _poses
    n_out = len(grid)
    rng = np.random.default_rng(6000 + n_in)
    uni = rng.uniform(-1.3, 1.3, size=(3000, n_in))
    corners = np.zeros((2 ** n_out, n_in))
    for k, sg in enumerate(itertools.product((-1, 1), repeat=n_out)):
        corners[k, :n_out] = [sd * (1 - 1.0 / n) for sd, n in zip(sg, grid)]
    out = np.full((6, n_in), 0.1)
    out[0, 0], out[1, -1] = np.nan, np.inf
    out[2:, 0] = (9.0, -9.0, 30.0, -1e30)
    rot, trans = (r32(a) for a in _poses(rng, 2, n_in, n_out))
    last = np.linalg.pinv(rot[1]) @ (np.asarray([1 - 1.0 / n for n in grid]) - trans[1])  # pose 1: the last cell
    pts = r32(np.concatenate([uni, corners, last[None], out]))
    P = len(pts)
    c = SimpleNamespace(grid=grid, P=P, B=2, points=pts, rot=rot, trans=trans, bg=r32(rng.normal(size=2)),
                        ow=r32(rng.uniform(0.5, 1.5, size=2)), pw=r32(rng.uniform(0.5, 1.5, size=P)),
                        g=r32(rng.normal(size=grid + (2,))))
    with np.errstate(invalid="ignore"):
        c.out = SR.raster_smooth(grid, pts, rot, trans, c.bg, c.ow, c.pw)
        c.pb = SR.raster_pullback_smooth(c.g, pts, rot, trans, c.ow, c.pw)
    frozen(c.points, c.rot, c.trans, c.bg, c.ow, c.pw, c.g, c.out, *c.pb)
    return c


@pytest.mark.parametrize("n_in,n_out,grid", EDGE_CASES)
def test_edge_grids_have_the_tiles_their_row_names(n_in, n_out, grid):
    """(CPU)  The tile count, the key bits the sort sees (ord_key_bits: the smallest `bits` with 2^bits - 1 >= tiles,
    so the all-ones key of a rejected point, masked, stays >= tiles) and the regime: under both poses rejected points
    and accepted points in the last tile; under the identity an accepted point in every corner cell."""
    nt = tile_count(grid)
    tiles = int(np.prod(nt))
    assert tiles == EDGE_GRIDS[grid]
    bits = 1
    while bits < 32 and 2 ** bits - 1 < tiles:
        bits += 1
    assert (tiles, bits) in ((1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4))
    assert (0xffffffff & (2 ** bits - 1)) >= tiles
    c = edge_case(n_in, grid)
    assert np.all(np.isfinite(c.out)) and all(np.all(np.isfinite(x)) for x in c.pb)
    n = np.asarray(grid)
    with np.errstate(invalid="ignore"):
        terms = list(SR._terms(grid, c.points, c.rot, c.trans, np.float64))
    for b, idx, j0, _w, _dw in terms:
        assert 0 < len(idx) < c.P, f"pose {b}: accepted and rejected points"
        tile = np.clip(j0, 0, n - 1) // np.asarray(TILE[n_out])
        assert np.all(tile == np.asarray(nt) - 1, axis=1).any(), f"pose {b}: no point in the last tile"
    # the identity pose: point 3000 + k is the centre of corner cell k
    _b, idx, j0, _w, _dw = terms[0]
    corners = np.arange(3000, 3000 + 2 ** n_out)
    pos = np.searchsorted(idx, corners)
    assert np.array_equal(idx[pos], corners), "a corner point is rejected"
    assert np.array_equal(j0[pos], [[0 if sd < 0 else n_d - 1 for sd, n_d in zip(sg, grid)]
                                    for sg in itertools.product((-1, 1), repeat=n_out)])


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid", EDGE_CASES)
def test_key_bit_and_small_grid_edges(dev, n_in, n_out, grid, npdt, tdt):
    c = edge_case(n_in, grid)
    args = dev_args(c, c, tdt, dev, c.B)
    need = dpr_amd.workspace_bytes_smooth("raster", grid, c.P, c.B, n_in, tdt, "tiled")
    assert need > 0
    assert dpr_amd.workspace_bytes_smooth("raster", grid, c.P, c.B, n_in, tdt, "atomic") == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tiled = dpr_amd.raster_smooth(grid, *args, algo="tiled", workspace=ws)
    atomic = dpr_amd.raster_smooth(grid, *args, algo="atomic")
    assert bool(torch.isfinite(tiled).all()) and bool(torch.isfinite(atomic).all())
    assert_close(tiled, c.out.astype(npdt), tol(npdt, "out"), f"{grid} tiled")
    assert_close(atomic, c.out.astype(npdt), tol(npdt, "out"), f"{grid} atomic")
    assert_close(tiled, atomic.cpu().numpy(), tol(npdt, "out"), f"{grid} tiled vs atomic")
    for b in range(c.B):  # plane by plane: a pose must not hide in the other's norm
        assert_close(tiled[..., b], c.out[..., b].astype(npdt), tol(npdt, "out"), f"{grid} tiled, pose {b}")
        assert_close(atomic[..., b], c.out[..., b].astype(npdt), tol(npdt, "out"), f"{grid} atomic, pose {b}")
    pb = dpr_amd.raster_pullback_smooth_(grid_to_dev(c.g.astype(npdt), dev), *args)
    for f, x in zip(FIELDS, pb):
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    check_pullback(pb, c.pb, npdt, f"{grid} ")
    assert not bool((pb.points[-6:] != 0).any()) and not bool((pb.point_weight[-6:] != 0).any())


# ------------------------------------------------------------------ A.7 the batch in one slice
LARGE_P = {524_033: (2048, 1), 523_776: (2046, 2)}  # P: (blocks of 256 points, slices of B = 3 poses)
LARGE_GRIDS = {2: (64, 64), 3: (32, 32, 32)}


def pose_slice_count(P, B):
    """Note 1 of include/dpr.h (SUMMATION ORDER): fewer than 2048 blocks of 256 points and B > 1 give up to
    min(B, ceil(2048 / blocks)) slices; from 2048 blocks on one slice."""
    blocks = -(-P // 256)
    if blocks >= 2048 or B == 1:
        return blocks, 1
    per_slice = -(-B // min(B, -(-2048 // blocks), 65535))
    return blocks, -(-B // per_slice)


def test_large_clouds_sit_on_both_sides_of_the_slice_threshold():
    for P, want in LARGE_P.items():
        assert pose_slice_count(P, 3) == want
    assert pose_slice_count(524_032, 3)[0] == 2047 and pose_slice_count(523_777, 3)[0] == 2047


@functools.lru_cache(maxsize=None)
def large_case(n):
    """(n, n) on LARGE_GRIDS[n], the larger cloud; the smaller one is its first 523 776 points.  Four poses: the
    tests of B = 3 take the first three."""
    from tests.test_smooth_gpu import _poses
    rng = np.random.default_rng(5200 + n)
    grid, B, P = LARGE_GRIDS[n], 4, max(LARGE_P)
    rot, trans = (r32(a) for a in _poses(rng, B, n, n))
    c = SimpleNamespace(grid=grid, B=B, points=r32(rng.uniform(-1.1, 1.1, size=(P, n))), rot=rot, trans=trans,
                        bg=r32(rng.normal(size=B)), ow=r32(rng.uniform(0.5, 1.5, size=B)),
                        pw=r32(rng.uniform(0.5, 1.5, size=P)), g=r32(rng.normal(size=grid + (B,))))
    frozen(c.points, c.rot, c.trans, c.bg, c.ow, c.pw, c.g)
    return c


@functools.lru_cache(maxsize=None)
def large_reference(n, P):
    c = large_case(n)
    return SR.raster_pullback_smooth(c.g[..., :3], c.points[:P], c.rot[:3], c.trans[:3], c.ow[:3], c.pw[:P])


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("P", list(LARGE_P))
@pytest.mark.parametrize("n", [2, 3])
def test_pullback_of_a_batch_at_the_slice_threshold(dev, n, P, npdt, tdt):
    """P = 524 033: one slice, one thread adds all poses in index order and stores once -- the reference, the same
    bits run to run, and the bits of (p0 + p1) + p2 of the three single-pose calls.  P = 523 776: two slices -- the
    reference, and the same bits run to run (two shares onto zero commute)."""
    c, B = large_case(n), 3
    slices = pose_slice_count(P, B)[1]
    assert slices == LARGE_P[P][1]
    g = grid_to_dev(c.g[..., :B].astype(npdt), dev)
    args = dev_args(c, c, tdt, dev, B, slice(0, P))
    pb = dpr_amd.raster_pullback_smooth_(g, *args)
    check_pullback(pb, large_reference(n, P), npdt, f"P={P} ")
    again = dpr_amd.raster_pullback_smooth_(g, *args)
    assert torch.equal(pb.points, again.points), "ds_dpoints differs between two runs"
    assert torch.equal(pb.point_weight, again.point_weight), "ds_dpoint_weight differs between two runs"
    if slices == 1:
        pts, rot, trans, bg, ow, pw = args
        one = [dpr_amd.raster_pullback_smooth_(g[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1], bg[b:b + 1],
                                               ow[b:b + 1], pw) for b in range(B)]
        assert torch.equal(pb.points, (one[0].points + one[1].points) + one[2].points), \
            "ds_dpoints is not (p0 + p1) + p2 of the single-pose calls"
        assert torch.equal(pb.point_weight, (one[0].point_weight + one[1].point_weight) + one[2].point_weight), \
            "ds_dpoint_weight is not (p0 + p1) + p2 of the single-pose calls"
        for b in range(B):  # (and a pose's own sums do not depend on the batch beyond their rounding)
            for f in ("rotation", "translation", "background", "out_weight"):
                assert_close(getattr(one[b], f)[0], getattr(pb, f)[b].cpu().numpy(), tol(npdt, "pose"),
                             f"pose {b} alone: {f}")


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n", [2, 3])
def test_one_slice_adds_four_poses_in_index_order(dev, n, npdt, tdt):
    """B = 4 at P = 524 033.  With three poses two slices of 2 + 1 poses add (p0 + p1) + p2 as well (two shares onto
    zero commute), so B = 3 cannot tell one slice from two; with four, two slices give (p0 + p1) + (p2 + p3) and only
    the one thread in index order gives ((p0 + p1) + p2) + p3."""
    c, B, P = large_case(n), 4, max(LARGE_P)
    assert pose_slice_count(P, B) == (2048, 1) and pose_slice_count(P - 1, B) == (2047, 2)
    g = grid_to_dev(c.g.astype(npdt), dev)
    pts, rot, trans, bg, ow, pw = dev_args(c, c, tdt, dev, B)
    pb = dpr_amd.raster_pullback_smooth_(g, pts, rot, trans, bg, ow, pw)
    one = [dpr_amd.raster_pullback_smooth_(g[..., b:b + 1], pts, rot[b:b + 1], trans[b:b + 1], bg[b:b + 1],
                                           ow[b:b + 1], pw) for b in range(B)]
    for f in ("points", "point_weight"):
        p = [getattr(x, f) for x in one]
        serial, paired = ((p[0] + p[1]) + p[2]) + p[3], (p[0] + p[1]) + (p[2] + p[3])
        assert not torch.equal(serial, paired), f"ds_d{f}: the two orders do not differ on this input"
        assert torch.equal(getattr(pb, f), serial), f"ds_d{f} is not ((p0 + p1) + p2) + p3 of the single-pose calls"


# ------------------------------------------------------------------ A.8 autograd
def ad_inputs(n_in, n_out, B, tdt, dev, requires=FIELDS):
    from tests.test_smooth_gpu import _poses
    rng = np.random.default_rng(8000 + 10 * n_in + n_out)
    P, grid = 50, (8,) * n_out
    rot, trans = _poses(rng, 2, n_in, n_out)
    vals = [rng.uniform(-1.1, 1.1, size=(P, n_in)), rot[:B], trans[:B], rng.normal(size=2)[:B],
            rng.uniform(0.5, 1.5, size=2)[:B], rng.uniform(0.5, 1.5, size=P)]
    xs = [to(r32(v), tdt, dev).requires_grad_(f in requires) for f, v in zip(FIELDS, vals)]
    return grid, xs, grid_to_dev(r32(rng.normal(size=grid + (2,)))[..., :B], dev).to(tdt)


def same(a, e, B, npdt, kind, what):
    if B == 1:
        assert torch.equal(a, e), what
    else:
        assert_close(a, e.cpu().numpy(), tol(npdt, kind), what)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 3), (3, 2)])
def test_autograd_equals_the_pullback(dev, n_in, n_out, B, algo, npdt, tdt):
    grid, xs, g = ad_inputs(n_in, n_out, B, tdt, dev)
    out = dpr_amd.raster_smooth_ad(grid, *xs, algo=algo)
    assert out.dtype == tdt and tuple(out.shape) == grid + (B,)
    (out * g).sum().backward()
    pb = dpr_amd.raster_pullback_smooth_(dpr_amd.to_grid_layout(g), *[x.detach() for x in xs])
    for f, kind, x, e in zip(FIELDS, KINDS, xs, pb):
        assert x.grad is not None and x.grad.dtype == tdt and x.grad.shape == x.shape, f
        same(x.grad, e, B, npdt, kind, f"{algo} B={B}: {f}.grad is not ds_d{f}")
    # point_weight = None and background = None: the defaults 1 and 0, the other gradients unchanged
    _, ys, _ = ad_inputs(n_in, n_out, B, tdt, dev)
    with torch.no_grad():
        ys[3].zero_()
        ys[5].fill_(1.0)
    (dpr_amd.raster_smooth_ad(grid, *ys, algo=algo) * g).sum().backward()
    _, zs, _ = ad_inputs(n_in, n_out, B, tdt, dev)
    out = dpr_amd.raster_smooth_ad(grid, zs[0], zs[1], zs[2], None, zs[4], None, algo=algo)
    (out * g).sum().backward()
    for i in (0, 1, 2, 4):
        same(zs[i].grad, ys[i].grad, B, npdt, KINDS[i], f"{algo} B={B}: {FIELDS[i]}.grad without the optional tensors")
    assert zs[3].grad is None and zs[5].grad is None
    # a subset of requires_grad
    _, rs, _ = ad_inputs(n_in, n_out, B, tdt, dev, requires=("rotation",))
    (dpr_amd.raster_smooth_ad(grid, *rs, algo=algo) * g).sum().backward()
    same(rs[1].grad, pb.rotation, B, npdt, "pose", f"{algo} B={B}: rotation.grad alone")
    assert all(rs[i].grad is None for i in (0, 2, 3, 4, 5))
