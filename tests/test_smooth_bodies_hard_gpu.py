"""The smooth splat of rigid bodies (k_smooth_bodies_* of csrc/dpr_smooth_bodies.hip: forward, pullback and forward
mode) in the regimes the other smooth families are held to: clustered clouds with cell-face, NaN / Inf and dropped
points held cell by cell and element by element, and the key bits of a group of images in the three drivers that loop
over groups (smooth_bodies_fwd_tiled, smooth_bodies_jvp_tiled, sample_smooth_bodies_image_tiled).

Every expectation is tests/smooth_bodies_reference.py (`BR`), tests/smooth_bodies_jvp_reference.py (`BJR`) or
tests/sample_smooth_bodies_reference.py (`SBR`) in fp64 on inputs rounded to fp32 once and used for both dtypes.

1  The hard body input, `bodies_input(name, order)`: smooth_input(name) of tests/test_smooth_hard_gpu.py (six border
points, the cluster, 64 cell-face points, 5 NaN / Inf points) with B = 3 images and K = 3 bodies, pose (b, k) the hard
pose (b + k) % 3 (every image sees every hard pose; body 0 is under the identity in image 0).  Labels: the border
points 0 0 1 1 2 2, the tail 0, the cluster three contiguous runs ("sorted") or default_rng(11).integers(0, 3)
("shuffled"); every 997th cluster point from the 97th on has a label of the cycle (-1, K, 2^31 - 1) and is dropped.
Counted on the CPU from the reference's cell choice on the smooth tiles (3-D 16 x 8 x 8, 2-D 64 x 16), per image
0 / 1 / 2 (test_hard_body_inputs_reach_the_regimes recounts the table and asserts the regimes):

    input, order      tiles   heaviest (image, tile) run   empty tiles       rejected          dropped
    H3 sorted         405     59 511 / 59 684 / 59 471     95 / 106 / 117    92 / 103 / 105    151
    H3 shuffled       405     59 463 / 59 582 / 59 621     90 / 113 / 121    84 / 104 / 112    151
    H2_22 sorted      10      31 455 / 31 456 / 31 379     0                 27 / 38 / 37      41
    H2_22 shuffled    10      31 442 / 31 457 / 31 391     0                 26 / 36 / 40      41
    H2_32 sorted      10      28 513 / 28 683 / 28 709     0                 29 / 37 / 44      41
    H2_32 shuffled    10      28 649 / 28 661 / 28 595     0                 30 / 35 / 45      41

The sorted body tensor is int64, the shuffled one int32.  Pullback outputs are caller buffers pre-filled with 7.5
(sorted) or NaN (shuffled).

2  Bounds.  Forward, fp32: |got - ref64| <= M_FACTOR rho E on EVERY cell, E the sum over the bodies of `budget_of`
(tests/test_smooth_hard_gpu.py) on the body's subset under its poses with the background counted once; fp64: tol(),
plane by plane.  Pullback: ds_dpoints and ds_dpoint_weight max |got - ref64| <= M_FACTOR rho max |ref64| (all rows,
and the 64 face rows alone); dropped and NaN / Inf rows exactly 0; pose gradients per (image, body) and ds_dout_weight
per image with tol().  Forward mode (V = 2): per plane (v, b), max |got - ref64| <= M_FACTOR rho max |ref64|.  Every
rho is the fp32 reference's own figure, measured on the CPU (test_recorded_rho_is_the_reference_s re-measures it):

    rho, CPU reference   forward     ds_dpoints B=1 / B=3     ds_dpoint_weight B=1 / B=3   out_dot all / point_weight
    H3 sorted            1.207e-06   1.182e-05 / 1.190e-05    8.915e-06 / 6.438e-06        8.032e-06 / 8.435e-06
    H3 shuffled          1.099e-06   1.305e-05 / 1.139e-05    9.230e-06 / 6.762e-06        9.423e-06 / 6.243e-06
    H2_22 sorted         5.259e-07   7.835e-06 / 8.088e-06    7.108e-06 / 7.666e-06        4.412e-06 / 4.161e-06
    H2_22 shuffled       5.259e-07   9.164e-06 / 7.481e-06    8.458e-06 / 6.921e-06        3.646e-06 / 3.421e-06
    H2_32 sorted         1.495e-06   9.152e-06 / 7.395e-06    9.837e-06 / 4.857e-06        3.969e-06 / 4.686e-06
    H2_32 shuffled       7.052e-07   9.152e-06 / 6.280e-06    9.834e-06 / 5.236e-06        4.218e-06 / 4.401e-06

A dropped point has the all-ones key whatever its coordinates, so the tiled kernels do the same work with NaN there;
include/dpr.h (SUMMATION ORDER) gives the tiled forward "f64 LDS atomics in arrival order ... float atomics in T:
rounding level, not bit-reproducible", so the two results are held to the any-order bound of the same <= 3^N partials
per cell, |a - b| <= 2 (3^N eps_T + P eps_64) E per cell (derived, not measured), and to the same bits on the far
cells.  test_dropped_points_with_nan_coordinates prints how many cells differ, and how many differ between two runs
of the same call.

3  Key bits of a group (`key_bodies`): KEY_CASES / KEY_GRIDS of tests/test_smooth_clouds_hard_gpu.py with one cloud of
P = 500 and K = 2 shuffled labels; test_key_bodies_are_what_the_cases_need asserts on the CPU that every image has
rejected points, the last tile of the last image of every group holds an accepted point, and one non-first image of a
group has an empty first tile (with one tile it accepts nothing).

Observed on an MI355X (the tests print them; fp32 unless noted, the bound m = M_FACTOR rho in brackets):

    forward, max |got - ref64| / E -- the same cell and figure on atomic and on tiled with max_pose_group 0 / 1 / 2,
    and on atomic with NaN in the dropped points
    H3      sorted 1.21e-06 (4.83e-06)   shuffled 7.47e-07 (4.40e-06)
    H2_22   sorted 8.32e-07 (2.10e-06)   shuffled 8.32e-07 (2.10e-06)
    H2_32   sorted 6.89e-07 (5.98e-06)   shuffled 7.05e-07 (2.82e-06)
    (H3 sorted and H2_32 shuffled: the reference's own worst cell, rho to three digits.)

    pullback, max |got - ref64| / max |ref64|    ds_dpoints B=1 / B=3                         ds_dpoint_weight B=1 / B=3
    H3 sorted         1.18e-05 (4.73e-05) / 1.35e-05 (4.76e-05)    1.05e-05 (3.57e-05) / 7.24e-06 (2.57e-05)
    H3 shuffled       1.30e-05 (5.22e-05) / 1.05e-05 (4.56e-05)    1.10e-05 (3.69e-05) / 8.20e-06 (2.71e-05)
    H2_22 sorted      1.12e-05 (3.13e-05) / 8.54e-06 (3.24e-05)    8.69e-06 (2.84e-05) / 8.14e-06 (3.07e-05)
    H2_22 shuffled    1.29e-05 (3.67e-05) / 8.79e-06 (2.99e-05)    9.12e-06 (3.38e-05) / 9.84e-06 (2.77e-05)
    H2_32 sorted      9.19e-06 (3.66e-05) / 7.47e-06 (2.96e-05)    1.08e-05 (3.94e-05) / 5.24e-06 (1.94e-05)
    H2_32 shuffled    1.02e-05 (3.66e-05) / 7.64e-06 (2.51e-05)    1.12e-05 (3.93e-05) / 5.23e-06 (2.09e-05)
    the 64 cell-face points alone: at most 3.95e-06; dropped and NaN / Inf rows: 0; fp64: at most 2.8e-14 everywhere.

    forward mode, max over the planes, the largest of atomic / tiled 0 / tiled 2 and B = 1 / 3
    H3       all 3.02e-06 (3.21e-05) sorted, 3.51e-06 (3.77e-05) shuffled; point_weight_dot 8.43e-06 (3.37e-05),
             6.14e-06 (2.50e-05)
    H2_22    all 3.12e-06 (1.76e-05), 2.77e-06 (1.46e-05); point_weight_dot 7.55e-06 (1.67e-05), 6.02e-06 (1.37e-05)
    H2_32    all 4.33e-06 (1.59e-05), 4.49e-06 (1.69e-05); point_weight_dot 6.20e-06 (1.87e-05), 7.03e-06 (1.76e-05)

    tiled with NaN in the dropped points against tiled without: H3 45 .. 121 (fp32) and 3 300 .. 4 500 (fp64) of
    1 010 100 cells differ, 2-D 0 .. 4 and 510 .. 670 of 21 000 -- and as many between two runs of the same call
    (H3 48 .. 79 and 3 800 .. 4 600); max |a - b| at most 3.7e-03 (fp32) and 1.1e-06 (fp64) of the bound.

Mutation record (scratch builds of libdpr outside the repository, one MI355X run of the three new modules each, every
module stopped at its first failure; every mutant keeps its accesses inside its buffers -- a wrong pose, image or
tangent index stays below B * K, B or V * B, a dropped deposit writes nothing -- and changes no loop bound upwards
and no barrier).  Each line: the mutant; the first test and assertion that failed in this module; the other modules.
  1 load_body_pose always takes the scalar       forward_cell_by_cell[H3-sorted-atomic-0-float64]: plane 0 against the
    branch (the first lane's body)                reference, 0.11 % off.  sample: values_one_by_one[H3-sorted-1-
                                                  float64], 2.6 % off; ranges: images_across_the_launch_cuts, out[.., 0],
                                                  26 % off
  2 k_smooth_bodies_keys takes the tile from     forward_cell_by_cell[H3-sorted-tiled-0-float64]: plane 1, 77 % off (the
    image b0, not b0 + bl                         two atomic cases pass before).  sample: pullback_element_by_element
                                                  [H3-sorted-3-tiled-0-float64], ds_dimage[.., 1] 85 % off; ranges:
                                                  tiled_forward_groups, out[.., 55925], 0.8 % off
  3 k_smooth_bodies_tile: `l < e[d] + 1`         forward_cell_by_cell[H3-sorted-tiled-0-float64]: plane 0, 6.9 % off.
                                                  sample: tiled_image_planes_are_the_tiled_splat (the splat side is the
                                                  mutant), 14 % off; ranges passes (one tile, no halo cell in the grid)
  4 k_smooth_bodies_tile_jvp: `vb = v * B + bl`  forward_mode_plane_by_plane[H3-sorted-tiled-2-3-all-float64]: planes
                                                  (0, 2) and (1, 2), the first image of the second group, 142 % and
                                                  108 % off (104 cases pass before it, tiled group 0 among them)
  5 k_sample_smooth_bodies_tile reads            key_bits_of_the_last_group_in_the_other_drivers[2-2-(1, 4, 3)-float64]:
    `ds_dvalues + b0 * P`                         ds_dimage[.., 2], 118 % off (330 cases of this module pass before).
                                                  sample: pullback_element_by_element[H3-sorted-3-tiled-0-float64],
                                                  ds_dimage[.., 1] 143 % off
  6 k_sample_smooth_bodies_bwd does not clear    passes this module and the sampling one (587 and 157 blocks of points:
    `tab[i]` after the flush                      three slices of ONE image, nothing to carry over).  ranges:
                                                  sample_smooth_bodies_images_across_the_launch_cuts[2-2-float32],
                                                  ds_drotation[65535, 0] 122 % off (slices of 65 images)
  7 smooth_bodies_jvp_atomic's kernel stops at   passes this module and the sampling one.  ranges: jvp_images_across_the
    image min(B, 65535) (no stride)               _launch_cuts[2-2-float32], out_dot[.., 0, 65535] 101 % off
None survived.  Argued, not run: a mutant that widens the LDS window (`l < e[d] + 3`), drops a `c < gd.n[d]` test or
the `p < 0 || p >= P` / `kb >= K` clamps, or lets the kernel of (7) run to 65535 with B below it, leaves its buffers.
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
from tests import smooth_reference as SR
from tests.test_parity_gpu import assert_close, grid_to_dev, tol
from tests.test_smooth_clouds_hard_gpu import (KEY_CASES, KEY_GRIDS, N_BORDER, empty_first_tile_pose, group_of,
                                               key_bits, tile_of)
from tests.test_smooth_hard_gpu import (DTYPES, INPUTS, M_FACTOR, N_BAD, N_FACE, TILE, budget_of, far_cells_of, frozen,
                                        r32, smooth_data, smooth_input, tile_count, to)

gpu = pytest.mark.gpu

ORDERS = ("sorted", "shuffled")
PAIRS = [(2, 2), (3, 3), (3, 2)]
NB = NK = 3  # images and bodies of the hard body input
DROP_LABELS = (-1, NK, 2 ** 31 - 1)
FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
VARIANTS = [("atomic", 0), ("tiled", 0), ("tiled", 1), ("tiled", 2)]  # algo, max_pose_group (2: groups of 2 + 1)
JVP_VARIANTS = [("atomic", 0), ("tiled", 0), ("tiled", 2)]
V = 2
TANGENT_KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
TANGENT_SETS = {"all": TANGENT_KINDS, "point_weight": ("point_weight",)}
FILL = {"sorted": 7.5, "shuffled": float("nan")}
# (input, order): per image (heaviest (image, tile) run, empty tiles, rejected points), and the dropped points
REGIMES = {
    ("H3", "sorted"): (((59511, 95, 92), (59684, 106, 103), (59471, 117, 105)), 151),
    ("H3", "shuffled"): (((59463, 90, 84), (59582, 113, 104), (59621, 121, 112)), 151),
    ("H2_22", "sorted"): (((31455, 0, 27), (31456, 0, 38), (31379, 0, 37)), 41),
    ("H2_22", "shuffled"): (((31442, 0, 26), (31457, 0, 36), (31391, 0, 40)), 41),
    ("H2_32", "sorted"): (((28513, 0, 29), (28683, 0, 37), (28709, 0, 44)), 41),
    ("H2_32", "shuffled"): (((28649, 0, 30), (28661, 0, 35), (28595, 0, 45)), 41),
}
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("H3", "sorted", "out"): 1.2072e-06,
    ("H3", "sorted", "points", 1): 1.1818e-05,
    ("H3", "sorted", "point_weight", 1): 8.9151e-06,
    ("H3", "sorted", "points", 3): 1.1897e-05,
    ("H3", "sorted", "point_weight", 3): 6.4384e-06,
    ("H3", "sorted", "jvp", "all"): 8.0325e-06,
    ("H3", "sorted", "jvp", "point_weight"): 8.4354e-06,
    ("H3", "shuffled", "out"): 1.0994e-06,
    ("H3", "shuffled", "points", 1): 1.3053e-05,
    ("H3", "shuffled", "point_weight", 1): 9.2295e-06,
    ("H3", "shuffled", "points", 3): 1.1392e-05,
    ("H3", "shuffled", "point_weight", 3): 6.7616e-06,
    ("H3", "shuffled", "jvp", "all"): 9.4226e-06,
    ("H3", "shuffled", "jvp", "point_weight"): 6.2434e-06,
    ("H2_22", "sorted", "out"): 5.2586e-07,
    ("H2_22", "sorted", "points", 1): 7.8346e-06,
    ("H2_22", "sorted", "point_weight", 1): 7.1077e-06,
    ("H2_22", "sorted", "points", 3): 8.0877e-06,
    ("H2_22", "sorted", "point_weight", 3): 7.6656e-06,
    ("H2_22", "sorted", "jvp", "all"): 4.4122e-06,
    ("H2_22", "sorted", "jvp", "point_weight"): 4.1614e-06,
    ("H2_22", "shuffled", "out"): 5.2586e-07,
    ("H2_22", "shuffled", "points", 1): 9.1638e-06,
    ("H2_22", "shuffled", "point_weight", 1): 8.4576e-06,
    ("H2_22", "shuffled", "points", 3): 7.4808e-06,
    ("H2_22", "shuffled", "point_weight", 3): 6.9206e-06,
    ("H2_22", "shuffled", "jvp", "all"): 3.6457e-06,
    ("H2_22", "shuffled", "jvp", "point_weight"): 3.4208e-06,
    ("H2_32", "sorted", "out"): 1.4953e-06,
    ("H2_32", "sorted", "points", 1): 9.1520e-06,
    ("H2_32", "sorted", "point_weight", 1): 9.8374e-06,
    ("H2_32", "sorted", "points", 3): 7.3954e-06,
    ("H2_32", "sorted", "point_weight", 3): 4.8566e-06,
    ("H2_32", "sorted", "jvp", "all"): 3.9687e-06,
    ("H2_32", "sorted", "jvp", "point_weight"): 4.6864e-06,
    ("H2_32", "shuffled", "out"): 7.0523e-07,
    ("H2_32", "shuffled", "points", 1): 9.1520e-06,
    ("H2_32", "shuffled", "point_weight", 1): 9.8342e-06,
    ("H2_32", "shuffled", "points", 3): 6.2801e-06,
    ("H2_32", "shuffled", "point_weight", 3): 5.2360e-06,
    ("H2_32", "shuffled", "jvp", "all"): 4.2182e-06,
    ("H2_32", "shuffled", "jvp", "point_weight"): 4.4014e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ 1 the hard body input (computed once)
@functools.lru_cache(maxsize=None)
def bodies_input(name, order):
    h = smooth_input(name)
    n = h.P - N_BORDER - N_FACE - N_BAD  # the cluster
    if order == "sorted":
        cluster = (np.arange(n) * NK) // n
    else:
        cluster = np.random.default_rng(11).integers(0, NK, n)
    cluster = cluster.astype(np.int64)
    at = np.arange(97, n, 997)
    cluster[at] = np.resize(DROP_LABELS, len(at))
    body = np.concatenate([[0, 0, 1, 1, 2, 2], cluster, np.zeros(N_FACE + N_BAD, np.int64)])
    pick = (np.arange(NB)[:, None] + np.arange(NK)[None, :]) % 3
    c = SimpleNamespace(name=name, order=order, n_in=h.n_in, n_out=h.n_out, grid=h.grid, P=h.P, B=NB, K=NK,
                        points=h.points, body=body, rot=np.ascontiguousarray(h.rot[pick]),
                        trans=np.ascontiguousarray(h.trans[pick]), dropped=at + N_BORDER)
    assert c.rot.shape == (NB, NK, h.n_out, h.n_in) and len(body) == h.P
    frozen(c.body, c.rot, c.trans, c.dropped)
    return c


def subsets(c):
    return [(k, np.flatnonzero(c.body == k)) for k in range(c.K)]


def cells_of(c):
    """(accepted (P, B) bool, j0 (P, B, N)) from the reference's cell choice under pose (b, body[p])"""
    acc, j0 = np.zeros((c.P, c.B), bool), np.zeros((c.P, c.B, c.n_out), np.int64)
    for k, idx in subsets(c):
        with np.errstate(invalid="ignore"):
            for b, i, cell, _w, _dw in SR._terms(c.grid, c.points[idx], c.rot[:, k], c.trans[:, k], np.float64):
                acc[idx[i], b], j0[idx[i], b] = True, cell
    return acc, j0


@functools.lru_cache(maxsize=None)
def hard_cells(name, order):
    return frozen(*cells_of(bodies_input(name, order)))


def body_to_dev(c, dev):
    return torch.as_tensor(np.array(c.body), device=dev).to(torch.int64 if c.order == "sorted" else torch.int32)


def dev_args(c, s, tdt, dev, B, points=None):
    """points, body, rotation, translation, background, out_weight, point_weight of the first B images"""
    t = lambda a: to(a, tdt, dev)
    return [t(c.points if points is None else points), body_to_dev(c, dev), t(c.rot[:B]), t(c.trans[:B]),
            t(s.bg[:B]), t(s.ow[:B]), t(s.pw)]


@functools.lru_cache(maxsize=None)
def reference_out(name, order, dtype=np.float64):
    c, s = bodies_input(name, order), smooth_data(name)
    with np.errstate(invalid="ignore"):
        out = BR.raster(c.grid, c.points, c.body, c.rot, c.trans, s.bg, s.ow, s.pw, dtype=dtype)
    assert np.all(np.isfinite(out))
    return frozen(out)


@functools.lru_cache(maxsize=None)
def reference_pullback(name, order, B, dtype=np.float64):
    c, s = bodies_input(name, order), smooth_data(name)
    with np.errstate(invalid="ignore"):
        pb = BR.raster_pullback(s.g[..., :B], c.points, c.body, c.rot[:B], c.trans[:B], s.ow[:B], s.pw, dtype=dtype)
    assert all(np.all(np.isfinite(x)) for x in pb)
    frozen(*pb)
    return pb


@functools.lru_cache(maxsize=None)
def budget(name, order):
    """E[c, b]: the sum over the bodies of budget_of on the body's subset, the background counted once"""
    c, s = bodies_input(name, order), smooth_data(name)
    E = np.broadcast_to(np.abs(s.bg), c.grid + (c.B,)).copy()
    for k, idx in subsets(c):
        E += budget_of(c.grid, c.points[idx], c.rot[:, k], c.trans[:, k], np.zeros(c.B), s.ow, s.pw[idx])
    assert np.all(E > 0)
    return frozen(E)


@functools.lru_cache(maxsize=None)
def far_cells(name, order):
    """grid + (B,) bool: no point of any body reaches the cell"""
    c = bodies_input(name, order)
    far = np.ones(c.grid + (c.B,), bool)
    for k, idx in subsets(c):
        far &= far_cells_of(c.grid, c.points[idx], c.rot[:, k], c.trans[:, k])
    return frozen(far)


@functools.lru_cache(maxsize=None)
def hard_tangents(name, order):
    """V = 2 tangents of every kind; NaN in the point tangents of the five NaN / Inf points and of the dropped ones"""
    c = bodies_input(name, order)
    rng = np.random.default_rng(4400 + len(name) + c.n_in + len(order))
    t = dict(points=rng.normal(size=(V, c.P, c.n_in)), rotation=rng.normal(size=(V, c.B, c.K, c.n_out, c.n_in)),
             translation=rng.normal(size=(V, c.B, c.K, c.n_out)), background=rng.normal(size=(V, c.B)),
             out_weight=rng.normal(size=(V, c.B)), point_weight=rng.normal(size=(V, c.P)))
    t = {k: r32(v) for k, v in t.items()}
    for k in ("points", "point_weight"):
        t[k][:, -N_BAD:] = np.nan
        t[k][:, c.dropped] = np.nan
    frozen(*t.values())
    return t


@functools.lru_cache(maxsize=None)
def reference_jvp(name, order, tangents, dtype=np.float64):
    """grid + (V, 3); the planes of the first image alone are [..., :1]"""
    c, s, t = bodies_input(name, order), smooth_data(name), hard_tangents(name, order)
    tan = {k + "_dot": t[k] for k in TANGENT_SETS[tangents]}
    with np.errstate(invalid="ignore"):
        out = BJR.raster_smooth_bodies_jvp(c.grid, c.points, c.body, c.rot, c.trans, s.ow, s.pw, V=V, dtype=dtype,
                                           **tan)
    assert np.all(np.isfinite(out))
    return frozen(out)


def device_jvp(c, s, t, kinds, B, tdt, dev, algo, group):
    tan = {}
    for k in kinds:
        v = t[k] if k in ("points", "point_weight") else t[k][:, :B]
        tan[k + "_dot"] = to(v, tdt, dev)
    pts, body, rot, trans, _bg, ow, pw = dev_args(c, s, tdt, dev, B)
    return dpr_amd.raster_smooth_bodies_jvp(c.grid, pts, body, rot, trans, None, ow, pw, tangents=V, algo=algo,
                                            max_pose_group=group, **tan)


def plane_ratios(got, ref64):
    """max |got - ref64| / max |ref64| of every plane (v, b): an array (V, B)"""
    axes = tuple(range(got.ndim - 2))
    return np.abs(got - ref64).max(axis=axes) / np.abs(ref64).max(axis=axes)


def measured_rho(name, order):
    """{key: rho} of the CPU reference, the keys of RHO."""
    r = {(name, order, "out"): float((np.abs(reference_out(name, order, np.float32).astype(np.float64)
                                             - reference_out(name, order)) / budget(name, order)).max())}
    for B in (1, 3):
        p64, p32 = reference_pullback(name, order, B), reference_pullback(name, order, B, np.float32)
        for field, i in (("points", 0), ("point_weight", 5)):
            r[(name, order, field, B)] = float(np.abs(p32[i].astype(np.float64) - p64[i]).max() / np.abs(p64[i]).max())
    for tangents in TANGENT_SETS:
        r[(name, order, "jvp", tangents)] = float(plane_ratios(
            reference_jvp(name, order, tangents, np.float32).astype(np.float64),
            reference_jvp(name, order, tangents)).max())
    return r


# ------------------------------------------------------------------ 1 the CPU side
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_hard_body_inputs_reach_the_regimes(name, order):
    """The table of the module docstring, recounted from the reference's cell choice per (image, body), and the
    regimes themselves: a change of the generator cannot drop one silently."""
    c = bodies_input(name, order)
    acc, j0 = hard_cells(name, order)
    tiles = int(np.prod(tile_count(c.grid)))
    assert tiles == {"H3": 405}.get(name, 10)
    valid = (c.body >= 0) & (c.body < c.K)
    dropped = np.flatnonzero(~valid)
    assert np.array_equal(dropped, c.dropped) and set(c.body[dropped]) == set(DROP_LABELS)
    assert np.array_equal(c.body[:N_BORDER], [0, 0, 1, 1, 2, 2]) and not c.body[-(N_FACE + N_BAD):].any()
    assert np.array_equal(c.rot[0, 0], np.eye(c.n_out, c.n_in)) and not c.trans[0, 0].any()
    for b in range(c.B):
        assert sorted(map(tuple, c.rot[b].reshape(c.K, -1))) == sorted(map(tuple, c.rot[0].reshape(c.K, -1)))
    n = np.asarray(c.grid)
    rows = []
    for b in range(c.B):
        a = np.flatnonzero(acc[:, b])
        counts = np.bincount(tile_of(c.grid, j0[a, b]), minlength=tiles)
        rejected = int((valid & ~acc[:, b]).sum())
        low, high = int((j0[a, b] == -1).any(axis=1).sum()), int((j0[a, b] == n).any(axis=1).sum())
        rows.append((int(counts.max()), int((counts == 0).sum()), rejected))
        print(f"{name} {order} image {b}: {tiles} tiles, heaviest run {counts.max()}, empty {rows[-1][1]}, rejected "
              f"{rejected}, dropped {len(dropped)}, j0 = -1: {low}, j0 = n: {high}")
        assert counts.max() > 256, (name, order, b)
        assert rejected >= N_BAD + 1, (name, order, b)
        if name == "H3":
            assert (counts == 0).any(), (name, order, b)
        if name != "H2_32" or b == 0:
            assert low > 0 and high > 0, (name, order, b)
        assert not acc[dropped, b].any()
    assert (tuple(rows), len(dropped)) == REGIMES[(name, order)]
    # a dropped point between two points that every image accepts
    inner = dropped[(dropped > 0) & (dropped < c.P - 1)]
    assert len(dropped) >= 1 and (acc[inner - 1].all(axis=1) & acc[inner + 1].all(axis=1)).any()
    # the tail of the cloud is what the tests below take it for
    assert np.all(~np.isfinite(c.points[-N_BAD:]).all(axis=1)) and np.all(np.isfinite(c.points[:-N_BAD]))
    # what wave_bodies sees: the labels of the blocks of 256 and of the waves of 64
    per = lambda size: [len(np.unique(c.body[i:i + size])) for i in range(0, c.P - size + 1, size)]
    blocks, waves = per(256), per(64)
    if order == "sorted":
        assert 1 in blocks, "no block of one label"
        assert any(blocks[w // 4] == 2 and waves[w] == 1 for w in range(4 * len(blocks))), \
            "no wave of one label inside a block of two"
        assert 2 in waves, "no wave of two labels"
    else:
        first, last = -(-N_BORDER // 64), (c.P - N_FACE - N_BAD) // 64  # the full waves of the cluster
        assert all(set(range(c.K)) <= set(c.body[64 * w:64 * w + 64]) for w in range(first, last))


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
def test_far_cells_hold_the_background_in_the_reference(name, order):
    """(CPU)  `far_cells` marks no cell a point of any body reaches: there the fp64 references are the background
    and the background tangent exactly, and every image has such cells."""
    far, out, s = far_cells(name, order), reference_out(name, order), smooth_data(name)
    assert all(far[..., b].any() for b in range(NB))
    assert np.array_equal(out[far], np.broadcast_to(s.bg, out.shape)[far])
    assert not np.array_equal(out, np.broadcast_to(s.bg, out.shape))
    t = hard_tangents(name, order)
    for tangents in TANGENT_SETS:
        ref = reference_jvp(name, order, tangents)
        want = np.broadcast_to(t["background"] if tangents == "all" else 0.0, ref.shape)
        mask = np.broadcast_to(far[..., None, :], ref.shape)
        assert np.array_equal(ref[mask], want[mask]) and not np.array_equal(ref, want)


# ------------------------------------------------------------------ 2a the forward, cell by cell
def check_cells_fp32(got, ref64, E, rho, what):
    m = M_FACTOR * rho
    ratio = np.abs(got - ref64) / E
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"{what}: max |got - ref64| / E = {ratio.max():.3e} (m = {m:.3e}) at {worst}")
    assert ratio.max() <= m, f"{what}: cell {worst}: |got - ref64| = {abs(got[worst] - ref64[worst]):.3e} > " \
        f"{m:.3e} * E = {m * E[worst]:.3e} ({int((ratio > m).sum())} cells over the bound)"


def check_far_cells(raw, far, want, what):
    bad = far & (raw != np.broadcast_to(want, raw.shape))
    assert far.any() and not bad.any(), f"{what}: {int(bad.sum())} of {int(far.sum())} far cells are not the " \
        f"background; first {tuple(int(v) for v in np.argwhere(bad)[0])}"


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo,group", VARIANTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_forward_cell_by_cell(dev, name, order, algo, group, npdt, tdt):
    c, s = bodies_input(name, order), smooth_data(name)
    ref64 = reference_out(name, order)
    out = dpr_amd.raster_smooth_bodies(c.grid, *dev_args(c, s, tdt, dev, c.B), algo=algo, max_pose_group=group)
    assert tuple(out.shape) == c.grid + (c.B,) and out.dtype == tdt
    raw = out.cpu().numpy()
    got = raw.astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out"
    what = f"{name} {order} {algo} group {group}"
    for b in range(c.B):
        assert_close(out[..., b], ref64[..., b].astype(npdt), tol(npdt, "out"), f"{what} plane {b}")
    if npdt == np.float32:
        check_cells_fp32(got, ref64, budget(name, order), RHO[(name, order, "out")], what)
    check_far_cells(raw, far_cells(name, order), s.bg.astype(npdt), what)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_dropped_points_with_nan_coordinates(dev, name, order, npdt, tdt):
    """NaN in the coordinates of the dropped points: the tiled planes stay what they were up to the order of the
    same partials (the bound of the module docstring; bit for bit on the far cells), the atomic result keeps its
    bound."""
    c, s = bodies_input(name, order), smooth_data(name)
    pts = np.array(c.points)
    pts[c.dropped] = np.nan
    ref64, E, far = reference_out(name, order), budget(name, order), far_cells(name, order)
    bound = 2 * (3 ** c.n_out * float(np.finfo(npdt).eps) + c.P * float(np.finfo(np.float64).eps)) * E
    for group in (0, 2):
        a = dpr_amd.raster_smooth_bodies(c.grid, *dev_args(c, s, tdt, dev, c.B), algo="tiled", max_pose_group=group)
        b = dpr_amd.raster_smooth_bodies(c.grid, *dev_args(c, s, tdt, dev, c.B, pts), algo="tiled",
                                         max_pose_group=group)
        again = dpr_amd.raster_smooth_bodies(c.grid, *dev_args(c, s, tdt, dev, c.B), algo="tiled",
                                             max_pose_group=group)
        a, b, again = a.cpu().numpy(), b.cpu().numpy(), again.cpu().numpy()
        assert np.all(np.isfinite(b)), "non-finite out"
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        print(f"{name} {order} tiled group {group} {np.dtype(npdt).name}: {int((a != b).sum())} of {a.size} cells "
              f"differ, max |a - b| / bound = {(d / bound).max():.3e}; two runs of the same call: "
              f"{int((a != again).sum())} cells differ")
        assert np.all(d <= bound), f"group {group}: {int((d > bound).sum())} cells move with NaN in the dropped points"
        assert np.array_equal(a[far], b[far])
    out = dpr_amd.raster_smooth_bodies(c.grid, *dev_args(c, s, tdt, dev, c.B, pts), algo="atomic")
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out"
    for b in range(c.B):
        assert_close(out[..., b], ref64[..., b].astype(npdt), tol(npdt, "out"), f"atomic plane {b}")
    if npdt == np.float32:
        check_cells_fp32(got, ref64, E, RHO[(name, order, "out")], f"{name} {order} atomic, NaN dropped points")


# ------------------------------------------------------------------ 2b the pullback, element by element
def filled_pullback(g, args, c, B, tdt, dev):
    """raster_pullback_smooth_bodies_ into caller buffers pre-filled with 7.5 (sorted) or NaN (shuffled)"""
    full = lambda *shape: torch.full(shape, FILL[c.order], dtype=tdt, device=dev)
    bufs = dict(ds_dpoints=full(c.P, c.n_in), ds_drotation=full(B, c.K, c.n_in, c.n_out).transpose(-1, -2),
                ds_dtranslation=full(B, c.K, c.n_out), ds_dbackground=full(B), ds_dout_weight=full(B),
                ds_dpoint_weight=full(c.P))
    pb = dpr_amd.raster_pullback_smooth_bodies_(g, *args, **bufs)
    for f, x in zip(FIELDS, pb):
        assert x.data_ptr() == bufs["ds_d" + f].data_ptr(), f"ds_d{f} is not the caller's buffer"
        assert bool(torch.isfinite(x).all()), f"non-finite ds_d{f}"
    return pb


def check_pose_gradients(pb, ref, npdt, what):
    """ds_drotation / ds_dtranslation per (image, body), ds_dout_weight per image, ds_dbackground"""
    B, K = ref[1].shape[:2]
    rtol = tol(npdt, "pose")
    for b in range(B):
        for k in range(K):
            assert_close(pb.rotation[b, k], ref[1][b, k].astype(npdt), rtol, f"{what}ds_drotation[{b}, {k}]")
            assert_close(pb.translation[b, k], ref[2][b, k].astype(npdt), rtol, f"{what}ds_dtranslation[{b}, {k}]")
        assert_close(pb.out_weight[b:b + 1], ref[4][b:b + 1].astype(npdt), rtol, f"{what}ds_dout_weight[{b}]")
    assert_close(pb.background, ref[3].astype(npdt), rtol, f"{what}ds_dbackground")


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_pullback_element_by_element(dev, name, order, B, npdt, tdt):
    c, s = bodies_input(name, order), smooth_data(name)
    ref = reference_pullback(name, order, B)
    assert dpr_amd.resolve_algo_smooth_bodies("pullback", c.grid, c.P, B, c.K, c.n_in) == "atomic"  # (its only one)
    pb = filled_pullback(grid_to_dev(s.g[..., :B].astype(npdt), dev), dev_args(c, s, tdt, dev, B), c, B, tdt, dev)
    what = f"{name} {order} B={B} "
    check_pose_gradients(pb, ref, npdt, what)
    faces = np.arange(c.P - N_BAD - N_FACE, c.P - N_BAD)
    for f, i in (("points", 0), ("point_weight", 5)):
        got, e = pb[i].cpu().numpy().astype(np.float64), ref[i]
        scale = np.abs(e).max()
        m = M_FACTOR * RHO[(name, order, f, B)] if npdt == np.float32 else tol(npdt, "points")
        d = np.abs(got - e).reshape(c.P, -1).max(axis=1)
        print(f"{what}{np.dtype(npdt).name} ds_d{f}: max |got - ref64| / max |ref64| = {d.max() / scale:.3e} "
              f"(m = {m:.3e}); face points {d[faces].max() / scale:.3e}")
        if npdt == np.float32:
            assert d.max() <= m * scale, f"ds_d{f}: max |got - ref64| = {d.max():.3e} > {m:.3e} * {scale:.3e} at " \
                f"point {int(d.argmax())}"
        else:
            assert_close(pb[i], e, tol(npdt, "points"), f"{what}ds_d{f}")
        over = np.nonzero(d[faces] > m * scale)[0]  # the cell-face points one by one
        assert len(over) == 0, f"ds_d{f} of face point {int(faces[over[0]])}: off by {d[faces][over[0]]:.3e} > " \
            f"{m:.3e} * {scale:.3e}; {len(over)} face points over the bound"
        assert not got[c.dropped].any(), f"ds_d{f} of a dropped point is not 0"
        assert not got[-N_BAD:].any(), f"ds_d{f} of a NaN / Inf point is not 0"


# ------------------------------------------------------------------ 2c forward mode, plane by plane
@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("tangents", list(TANGENT_SETS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("algo,group", JVP_VARIANTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_forward_mode_plane_by_plane(dev, name, order, algo, group, B, tangents, npdt, tdt):
    c, s, t = bodies_input(name, order), smooth_data(name), hard_tangents(name, order)
    ref64 = reference_jvp(name, order, tangents)[..., :B]
    out = device_jvp(c, s, t, TANGENT_SETS[tangents], B, tdt, dev, algo, group)
    assert tuple(out.shape) == c.grid + (V, B) and out.dtype == tdt
    raw = out.cpu().numpy()
    got = raw.astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out_dot: a NaN tangent of a dropped or NaN / Inf point was used"
    what = f"{name} {order} {algo} group {group} B={B} {tangents} {np.dtype(npdt).name}"
    ratio = plane_ratios(got, ref64)
    m = M_FACTOR * RHO[(name, order, "jvp", tangents)] if npdt == np.float32 else 1e-10
    print(f"{what}: max |got - ref64| / max |ref64| over the planes = {ratio.max():.3e} (m = {m:.3e})")
    assert ratio.max() <= m, f"{what}: plane (v, b) = {np.unravel_index(int(ratio.argmax()), ratio.shape)} is " \
        f"{ratio.max():.3e} > {m:.3e} off"
    far = np.broadcast_to(far_cells(name, order)[..., None, :B], got.shape)
    want = (t["background"][:, :B] if tangents == "all" else np.zeros((V, B))).astype(npdt)
    check_far_cells(raw, far, want, what)


# ------------------------------------------------------------------ 3 the key bits of a group
KEY_P, KEY_K, KEY_BAD = 500, 2, 4
KEY_PARAMS = [(n_in, n_out, case) for case in KEY_CASES for n_in, n_out in PAIRS]
# the cases whose last group sorts on other bits than the full one: every driver's own group loop
KEY_PARAMS_LAST = [p for p in KEY_PARAMS if KEY_CASES[p[2]][0][1] != KEY_CASES[p[2]][1][1]]


@functools.lru_cache(maxsize=None)
def key_bodies(n_in, n_out, case):
    """One cloud of 500 points uniform in +-1.3 with K = 2 shuffled labels, its last four rows NaN / Inf (rejected in
    every image); image b under two poses of their own.  Row 10 + b is the centre of the last cell under its pose of
    image b; the hollow image's poses are scaled and shifted to put the whole cloud beyond the first tile on axis 0
    (with one tile: beyond the grid)."""
    from tests.test_smooth_clouds_gpu import _poses
    tiles, B, max_group = case
    grid = KEY_GRIDS[tiles][n_out]
    n = np.asarray(grid, np.float64)
    rng = np.random.default_rng(5400 + 100 * n_in + 10 * n_out + sum(case))
    P, K = KEY_P, KEY_K
    rot, trans = _poses(rng, B * K, n_in, n_out)
    rot, trans = rot.reshape(B, K, n_out, n_in), trans.reshape(B, K, n_out)
    hollow = empty_first_tile_pose(tiles, B, max_group)
    if hollow is not None:
        if tiles == 1:
            trans[hollow, :, 0] += 5.0
        else:
            lo, hi = TILE[n_out][0] + 0.5, n[0] + 1.0
            rot[hollow] *= 0.45 * (hi - lo) / (1.3 * np.sqrt(n_in) * n[0] / 2)
            trans[hollow] = 0.0
            trans[hollow, :, 0] = (lo + hi) / n[0] - 1.0
    pts = rng.uniform(-1.3, 1.3, size=(P, n_in))
    body = rng.integers(0, K, P)
    for b in range(B):
        if not (b == hollow and tiles == 1):  # (far outside every other image where the hollow pose is scaled)
            r, t = rot[b, body[10 + b]], trans[b, body[10 + b]]
            pts[10 + b] = np.linalg.pinv(r) @ ((-1 + 2 * (n - 0.5) / n) - t)
    pts[-KEY_BAD:] = 0.1
    pts[-4, 0], pts[-3, -1], pts[-2, 0], pts[-1, -1] = np.nan, np.inf, -np.inf, np.nan
    c = SimpleNamespace(n_in=n_in, n_out=n_out, grid=grid, P=P, B=B, K=K, tiles=tiles, max_group=max_group,
                        hollow=hollow, order="sorted", points=r32(pts), body=body.astype(np.int64), rot=r32(rot),
                        trans=r32(trans), bg=r32(rng.normal(size=B)), ow=r32(rng.uniform(0.5, 1.5, size=B)),
                        pw=r32(rng.uniform(0.5, 1.5, size=P)), dv=r32(rng.normal(size=(P, B))))
    t = dict(points=rng.normal(size=(V, P, n_in)), rotation=rng.normal(size=(V, B, K, n_out, n_in)),
             translation=rng.normal(size=(V, B, K, n_out)), background=rng.normal(size=(V, B)),
             out_weight=rng.normal(size=(V, B)), point_weight=rng.normal(size=(V, P)))
    c.t = {k: r32(v) for k, v in t.items()}
    c.t["points"][:, -KEY_BAD:] = np.nan
    c.t["point_weight"][:, -KEY_BAD:] = np.nan
    frozen(c.points, c.body, c.rot, c.trans, c.bg, c.ow, c.pw, c.dv, *c.t.values())
    return c


@functools.lru_cache(maxsize=None)
def key_reference(n_in, n_out, case, what):
    c = key_bodies(n_in, n_out, case)
    with np.errstate(invalid="ignore"):
        if what == "out":
            r = BR.raster(c.grid, c.points, c.body, c.rot, c.trans, c.bg, c.ow, c.pw)
        elif what == "jvp":
            r = BJR.raster_smooth_bodies_jvp(c.grid, c.points, c.body, c.rot, c.trans, c.ow, c.pw, V=V,
                                             **{k + "_dot": v for k, v in c.t.items()})
        else:  # ds_dimage does not depend on the image
            r = SBR.sample_pullback(c.dv, np.zeros(c.grid + (c.B,)), c.points, c.body, c.rot, c.trans)[0]
    assert np.all(np.isfinite(r))
    return frozen(r)


@pytest.mark.parametrize("n_in,n_out,case", KEY_PARAMS)
def test_key_bodies_are_what_the_cases_need(n_in, n_out, case):
    """(CPU)  Every image has rejected points (the run of the all-ones keys is never empty); the last tile of the
    last image of every group holds an accepted point (its run touches that run); one non-first image of a group has
    an empty first tile (a start-table entry shared with the image before it) -- with one tile it accepts nothing."""
    c = key_bodies(n_in, n_out, case)
    nb = group_of(c.B, c.max_group)
    last = c.B % nb or nb
    assert ((nb * c.tiles, key_bits(nb * c.tiles)), (last * c.tiles, key_bits(last * c.tiles))) == KEY_CASES[case]
    assert set(c.body) == {0, 1} and len(np.unique(c.body[:64])) == 2
    acc, j0 = cells_of(c)
    for b in range(c.B):
        a = np.flatnonzero(acc[:, b])
        tile = tile_of(c.grid, j0[a, b])
        assert len(a) < c.P, f"image {b}: no rejected point"
        if b % nb == nb - 1 or b == c.B - 1:
            assert (tile == c.tiles - 1).any(), f"image {b}, the last of its group: nothing in the last tile"
        if b == c.hollow:
            assert 0 < b % nb and not (tile == 0).any() and (len(a) > 0) == (c.tiles > 1)
        else:
            assert len(a) > 0 and {0, 1} == set(c.body[a])
    assert (c.hollow is not None) == (nb >= (3 if c.tiles == 1 else 2))
    assert {(1, 4, 3), (3, 4, 3), (4, 5, 4), (7, 3, 2)} <= {p[2] for p in KEY_PARAMS_LAST}


def key_args(c, tdt, dev):
    t = lambda a: to(a, tdt, dev)
    return [t(c.points), body_to_dev(c, dev), t(c.rot), t(c.trans), t(c.bg), t(c.ow), t(c.pw)]


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,case", KEY_PARAMS)
def test_key_bits_of_a_group(dev, n_in, n_out, case, npdt, tdt):
    c = key_bodies(n_in, n_out, case)
    ref = key_reference(n_in, n_out, case, "out")
    args = key_args(c, tdt, dev)
    tiled = dpr_amd.raster_smooth_bodies(c.grid, *args, algo="tiled", max_pose_group=c.max_group)
    atomic = dpr_amd.raster_smooth_bodies(c.grid, *args, algo="atomic")
    assert bool(torch.isfinite(tiled).all()) and bool(torch.isfinite(atomic).all())
    for b in range(c.B):  # plane by plane: an image must not hide in the others' norm
        e = ref[..., b].astype(npdt)
        assert_close(tiled[..., b], e, tol(npdt, "out"), f"{case} tiled, image {b}")
        assert_close(atomic[..., b], e, tol(npdt, "out"), f"{case} atomic, image {b}")
        assert_close(tiled[..., b], atomic[..., b].cpu().numpy(), tol(npdt, "out"), f"{case} tiled vs atomic, {b}")
    if c.hollow is not None and c.tiles == 1:  # an image nothing is accepted in: exactly its background
        assert bool((tiled[..., c.hollow] == float(c.bg[c.hollow].astype(npdt))).all())


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,case", KEY_PARAMS_LAST)
def test_key_bits_of_the_last_group_in_the_other_drivers(dev, n_in, n_out, case, npdt, tdt):
    """smooth_bodies_jvp_tiled (V = 2, all tangents) and the image planes of sample_smooth_bodies_pullback_ on
    tiled: each has its own loop over the groups."""
    c = key_bodies(n_in, n_out, case)
    pts, body, rot, trans, _bg, ow, pw = key_args(c, tdt, dev)
    tan = {k + "_dot": to(v, tdt, dev) for k, v in c.t.items()}
    out = dpr_amd.raster_smooth_bodies_jvp(c.grid, pts, body, rot, trans, None, ow, pw, tangents=V, algo="tiled",
                                           max_pose_group=c.max_group, **tan)
    ref = key_reference(n_in, n_out, case, "jvp")
    assert tuple(out.shape) == c.grid + (V, c.B) and bool(torch.isfinite(out).all())
    rtol = 1e-10 if npdt == np.float64 else 1e-4  # (norm-wise per plane: tests/test_smooth_bodies_jvp_gpu.py's)
    for v in range(V):
        for b in range(c.B):
            assert_close(out[..., v, b], ref[..., v, b].astype(npdt), rtol, f"{case} out_dot plane ({v}, {b})")
    d_img = dpr_amd.empty_grid(c.grid, c.B, tdt, dev).fill_(float("nan"))
    pb = dpr_amd.sample_smooth_bodies_pullback_(to(c.dv.T, tdt, dev).t(), None, pts, body, rot, trans,
                                                ds_dimage=d_img, need=("image",), algo="tiled",
                                                max_pose_group=c.max_group)
    assert pb.image is d_img and bool(torch.isfinite(d_img).all())
    ref = key_reference(n_in, n_out, case, "image")
    for b in range(c.B):
        assert_close(d_img[..., b], ref[..., b].astype(npdt), tol(npdt, "out"), f"{case} ds_dimage[.., {b}]")
        if b == c.hollow and c.tiles == 1:
            assert not bool((d_img[..., b] != 0).any())
