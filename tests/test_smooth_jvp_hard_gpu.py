"""The forward-mode derivative of the smooth splat (k_smooth_jvp_atomic / k_smooth_tile_jvp of csrc/dpr_smooth.hip) in
the hard regimes: every lane pattern the wave combine of the atomic kernel can meet, held deposit by deposit; the
clustered inputs of tests/test_smooth_hard_gpu.py with cell-face and NaN / Inf points, plane by plane; and the key-bit
and small-grid edges of the tiled path.

Every expectation is tests/smooth_jvp_reference.py (`JR`) in fp64 on inputs rounded to fp32 once.

1a  The wave patterns.  Grids (8, 8) and (8, 8, 8), B = 2 (pose 0 the identity, pose 1 generic), K = 3, all six
tangents.  Point p is lane p % 64 of wave p // 64; every point is a cell's centre plus at most +-0.3 cell.  Under the
identity pose the waves are, with what the kernel's rule (a search only from kSmJvpMinRun = 8 lanes that equal their
neighbour on; at most kSmJvpTries = 8 cells tried; at most kSmJvpGroups = 4 groups) makes of them --
test_wave_patterns_reach_the_combine_s_branches rebuilds this table from the reference's j0:

    wave  lanes                                                   equal neighbours   groups (lead order)   solo lanes
    0     64 in one cell                                          63                 64                    0
    1     4 cells x 16                                            60                 16 16 16 16           0
    2     5 cells x 12, 4 singles                                 55                 12 12 12 12           16
    3     8 singles, 56 in one cell                               55                 none (tries used)     64
    4     7 singles, 57 in one cell                               56                 57 (eighth try)       7
    5     a run of 8 in lanes 20..27, the rest distinct           7                  none (no search)      64
    6     a run of 9 in lanes 3..11, the rest distinct            8                  9 (fourth try)        55
    7     A B A B ...                                             0                  none (no search)      64
    8     10 x A, then A on every third lane among distinct       9                  28 (with gaps)        36
    9     one cell, lanes 0, 5, .. rejected (far / NaN / Inf)     38                 51                    0
    10    32 with j0 = -1 on axis 0, 32 with j0 = n on the last   62                 32 32                 0
    11    every lane rejected                                     0                  none                  0
    12    20 in one cell (P % 64 = 20: 44 lanes not live)         19                 20                    0

The fp64 bound is derived, not measured: |got - ref64| <= (n_c + 16) eps A_c on every cell of every plane, n_c the
deposits on the cell, A_c the sum of their absolute values plus |background_dot| (JR with magnitudes=True): the
any-order worst case of the additions with 16 roundings for a deposit's own arithmetic.  One lost or doubled deposit
is ~1e-1 A_c.  The fp32 bound is per plane (k, b): max |got - ref64| <= M_FACTOR rho max |ref64|, rho the fp32
reference's own figure (the largest over the planes), measured on the CPU (test_recorded_rho_is_the_reference_s).

1b  hard inputs H3 / H2_22 / H2_32 (`smooth_input`), K = 2, B in (1, 3), all tangents and point_weight_dot alone;
the same per-plane bound; cells nothing reaches hold background_dot[k, b] exactly; the five NaN / Inf points carry NaN
tangents.  1c  `edge_case` on every EDGE_GRIDS entry, K = 3, B = 2, plane by plane.

    rho, CPU reference    all tangents    point_weight_dot alone
    waves (2,2)           4.592e-07
    waves (3,3)           3.373e-07
    waves (3,2)           4.779e-07
    H3                    2.199e-05       7.769e-06
    H2_22                 7.121e-06       4.863e-06
    H2_32                 5.166e-06       5.278e-06
    (H3, all tangents: plane (k, b) = (0, 2), whose worst cell holds -1.4e4 as the sum of the cluster's deposits of
    both signs; the fp32 reference is 0.53 off there.  The other five planes: 7.0e-06 .. 1.2e-05.)

Observed on an MI355X (the tests print them):

    waves, fp64: max |got - ref64| / ((n_c + 16) eps A_c)    atomic as built / permuted    tiled as built / permuted
    (2,2)                                                    5.3e-02 / 2.7e-02             3.7e-02 / 4.8e-02
    (3,3)                                                    2.1e-01 / 2.1e-01             2.1e-01 / 2.1e-01
    (3,2)                                                    3.3e-02 / 3.5e-02             3.1e-02 / 3.5e-02
    ((3,3): the same cell (2, 7, 7) of plane (1, 0) on all four paths.)
    waves, fp32: max over the planes of max |got - ref64| / max |ref64| (m)
    (2,2)   4.3e-07 / 3.8e-07 / 3.9e-07 / 3.9e-07 (1.84e-06)    (3,3)   4.7e-07 everywhere (1.35e-06)
    (3,2)   5.7e-07 / 5.2e-07 / 5.7e-07 / 5.7e-07 (1.91e-06)

    hard inputs, fp32, the same ratio (m)    atomic B=1 / B=3       tiled B=1 / B=3
    H3, all (8.80e-05)                       4.01e-06 / 5.86e-06    1.40e-06 / 2.03e-06
    H3, point_weight_dot (3.11e-05)          7.43e-06 / 7.91e-06    6.61e-06 / 6.64e-06
    H2_22, all (2.85e-05)                    1.80e-06 / 2.78e-06    7.05e-07 / 2.45e-06
    H2_22, point_weight_dot (1.95e-05)       2.55e-06 / 5.56e-06    2.20e-06 / 5.77e-06
    H2_32, all (2.07e-05)                    3.38e-06 / 3.97e-06    9.78e-07 / 2.16e-06
    H2_32, point_weight_dot (2.11e-05)       3.16e-06 / 6.00e-06    4.14e-06 / 6.11e-06

Mutation record (scratch builds of libdpr, one MI355X run of this module each; both mutants keep every access
inside the buffers: they change which lanes issue an atomic, not where):
  k_smooth_jvp_atomic without `solo &= ~m`       wave_patterns_deposit_by_deposit[2-2-atomic-as built-float64]: the
  (the lanes of a group deposit on their own     bound per cell, cell (7, 0) of plane (2, 1) 1.5e+01 off against
  as well)                                       1.6e-13 (20 deposits, A = 1.9e+01); 354 cells over the bound
  k_smooth_jvp_atomic's search without           the same case and assertion: cell (0, 6) of plane (1, 1) 1.1e+02 off
  `ng < kSmJvpGroups` (a fifth group             against 3.2e-12 (95 deposits, A = 1.3e+02); 156 cells over the bound
  overwrites gm3)
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from tests import smooth_jvp_reference as JR
from tests import smooth_reference as SR
from tests.test_parity_gpu import assert_close
from tests.test_smooth_hard_gpu import (DTYPES, EDGE_CASES, INPUTS, M_FACTOR, N_BAD, edge_case, far_cells, frozen, r32,
                                        smooth_input, smooth_data, to)

gpu = pytest.mark.gpu

PAIRS = [(2, 2), (3, 3), (3, 2)]
ALGOS = ("atomic", "tiled")
KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
TANGENT_SETS = {"all": KINDS, "point_weight": ("point_weight",)}
# the constants of k_smooth_jvp_atomic (csrc/dpr_smooth.hip)
WAVE, GROUPS, TRIES, MIN_RUN = 64, 4, 8, 8
# wave: (lanes equal to their neighbour, group sizes in lead order, solo lanes) under the identity pose
WAVE_PLAN = [(63, [64], 0), (60, [16, 16, 16, 16], 0), (55, [12, 12, 12, 12], 16), (55, [], 64), (56, [57], 7),
             (7, [], 64), (8, [9], 55), (0, [], 64), (9, [28], 36), (38, [51], 0), (62, [32, 32], 0), (0, [], 0),
             (19, [20], 0)]
# rho of the module docstring (CPU reference); the bounds are M_FACTOR * rho
RHO = {
    ("waves", 2, 2): 4.5915e-07,
    ("waves", 3, 3): 3.3725e-07,
    ("waves", 3, 2): 4.7793e-07,
    ("H3", "all"): 2.1994e-05,
    ("H3", "point_weight"): 7.7685e-06,
    ("H2_22", "all"): 7.1212e-06,
    ("H2_22", "point_weight"): 4.8629e-06,
    ("H2_32", "all"): 5.1661e-06,
    ("H2_32", "point_weight"): 5.2775e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def jvp_tol(npdt):
    """norm-wise against the reference: tests/test_smooth_jvp_gpu.py's"""
    return 1e-10 if npdt == np.float64 else 1e-4


def make_tangents(rng, K, B, P, n_in, n_out):
    t = dict(points=rng.normal(size=(K, P, n_in)), rotation=rng.normal(size=(K, B, n_out, n_in)),
             translation=rng.normal(size=(K, B, n_out)), background=rng.normal(size=(K, B)),
             out_weight=rng.normal(size=(K, B)), point_weight=rng.normal(size=(K, P)))
    return {k: r32(v) for k, v in t.items()}


def freeze_all(t):
    for v in t.values():
        v.setflags(write=False)
    return t


def reference(c, t, kinds, B, dtype=np.float64, **kw):
    """JR on the first B poses of case c (grid, points, rot, trans, ow, pw) along the tangents `kinds` of t."""
    K = t["points"].shape[0]
    tans = {k + "_dot": (t[k] if k in ("points", "point_weight") else t[k][:, :B]) for k in kinds}
    with np.errstate(invalid="ignore"):
        return JR.raster_smooth_jvp(c.grid, c.points, c.rot[:B], c.trans[:B], c.ow[:B], c.pw, K=K, dtype=dtype, **tans,
                                    **kw)


def device_jvp(c, t, kinds, B, tdt, dev, algo, keep=slice(None), order=None):
    """dpr_amd.raster_smooth_jvp on the first B poses; `keep` / `order` select or permute the points."""
    sel = (lambda a, axis: np.take(a, order, axis=axis)) if order is not None else \
        (lambda a, axis: a[keep] if axis == 0 else a[:, keep])
    K = t["points"].shape[0]
    tans = {}
    for k in kinds:
        v = sel(t[k], 1) if k in ("points", "point_weight") else t[k][:, :B]
        tans[k + "_dot"] = to(v, tdt, dev)
    t = lambda a: to(a, tdt, dev)
    return dpr_amd.raster_smooth_jvp(c.grid, t(sel(c.points, 0)), t(c.rot[:B]), t(c.trans[:B]), None, t(c.ow[:B]),
                                     t(sel(c.pw, 0)), tangents=K, algo=algo, **tans)


def plane_ratios(got, ref64):
    """max |got - ref64| / max |ref64| of every plane (k, b): an array (K, B)"""
    axes = tuple(range(got.ndim - 2))
    return np.abs(got - ref64).max(axis=axes) / np.abs(ref64).max(axis=axes)


def check_planes_fp32(got, ref64, rho, what):
    ratio = plane_ratios(got, ref64)
    m = M_FACTOR * rho
    print(f"{what}: max |got - ref64| / max |ref64| over the planes = {ratio.max():.3e} (m = {m:.3e})")
    assert ratio.max() <= m, f"{what}: plane (k, b) = {np.unravel_index(int(ratio.argmax()), ratio.shape)} is " \
        f"{ratio.max():.3e} > {m:.3e} off"


def check_planes_fp64(out, ref64, what):
    K, B = ref64.shape[-2:]
    for k in range(K):
        for b in range(B):
            assert_close(out[..., k, b], ref64[..., k, b], jvp_tol(np.float64), f"{what} plane ({k}, {b})")


# ------------------------------------------------------------------ 1a the wave patterns
def wave_lanes(n_out, rng):
    """The waves of the module docstring: per wave a list of cells (tuples; -1 and n occur) or of "far" / "nan" /
    "inf" for a rejected lane."""
    n = 8
    cells = [tuple(int(v) for v in c) for c in rng.permutation(list(itertools.product(range(n), repeat=n_out)))]

    def distinct(count, avoid=()):
        pool = [c for c in rng.permutation(cells).tolist() if tuple(c) not in avoid]
        assert len(pool) >= count
        return [tuple(c) for c in pool[:count]]

    bad = ("far", "nan", "inf")
    own = iter(cells)  # a wave's packed cells are its own: the permuted cloud has no runs to speak of
    waves = [[next(own)] * 64]
    waves.append([c for c in (next(own) for _ in range(4)) for _ in range(16)])
    five = [next(own) for _ in range(5)]
    waves.append([c for c in five for _ in range(12)] + distinct(4, avoid=five))
    for singles in (8, 7):
        A = next(own)
        waves.append(distinct(singles, avoid=(A,)) + [A] * (64 - singles))
    for at, run in ((20, 8), (3, 9)):
        A = next(own)
        rest = distinct(64 - run, avoid=(A,))
        waves.append(rest[:at] + [A] * run + rest[at:])
    waves.append([next(own), next(own)] * 32)
    A = next(own)
    rest = iter(distinct(36, avoid=(A,)))
    waves.append([A] * 10 + [A if lane % 3 == 0 else next(rest) for lane in range(10, 64)])
    A = next(own)
    waves.append([bad[(lane // 5) % 3] if lane % 5 == 0 else A for lane in range(64)])
    waves.append([(-1,) + next(own)[1:]] * 32 + [next(own)[:-1] + (n,)] * 32)
    waves.append([bad[lane % 3] for lane in range(64)])
    waves.append([next(own)] * 20)
    return waves


@functools.lru_cache(maxsize=None)
def pattern_case(n_in, n_out):
    from tests.test_smooth_gpu import _poses
    rng = np.random.default_rng(4100 + 10 * n_in + n_out)
    grid, B, K = (8,) * n_out, 2, 3
    lanes = [c for w in wave_lanes(n_out, rng) for c in w]
    P = len(lanes)
    pts = rng.uniform(-0.9, 0.9, size=(P, n_in))
    for p, c in enumerate(lanes):
        if c == "far":
            pts[p, 0] = 9.0
        elif c == "nan":
            pts[p, 0] = np.nan
        elif c == "inf":
            pts[p, -1] = np.inf
        else:
            pts[p, :n_out] = -1 + 2 * (np.asarray(c) + 0.5 + rng.uniform(-0.3, 0.3, size=n_out)) / 8
    rot, trans = (r32(a) for a in _poses(rng, B, n_in, n_out))
    c = SimpleNamespace(n_in=n_in, n_out=n_out, grid=grid, P=P, B=B, K=K, lanes=lanes, points=r32(pts), rot=rot,
                        trans=trans, ow=r32(rng.uniform(0.5, 1.5, size=B)), pw=r32(rng.uniform(0.5, 1.5, size=P)))
    t = make_tangents(rng, K, B, P, n_in, n_out)
    c.rejected = np.ones(P, bool)  # by every pose
    with np.errstate(invalid="ignore"):
        for _b, idx, *_ in SR._terms(grid, c.points, rot, trans, np.float64):
            c.rejected[idx] = False
    t["points"][:, c.rejected] = np.nan
    t["point_weight"][:, c.rejected] = np.nan
    c.t = freeze_all(t)
    c.perm = np.random.default_rng(41).permutation(P)
    c.ref = reference(c, c.t, KINDS, B)
    c.A, c.n = reference(c, c.t, KINDS, B, magnitudes=True)
    assert np.all(np.isfinite(c.ref)) and np.all(np.isfinite(c.A))
    frozen(c.points, c.rot, c.trans, c.ow, c.pw, c.ref, c.A, c.n)
    return c


def wave_plan(ok, j0):
    """k_smooth_jvp_atomic's rule on one wave: ok (64,) bool, j0 (64, N) -> (lanes equal to their neighbour, group
    sizes in lead order, solo lanes)."""
    same = lambda a, b: bool(ok[a] and ok[b] and np.array_equal(j0[a], j0[b]))
    run = sum(same(lane, lane - 1) for lane in range(1, WAVE))
    solo, groups = set(np.nonzero(ok)[0].tolist()), []
    if run >= MIN_RUN:
        todo = sorted(solo)
        for _try in range(TRIES):
            if not todo or len(groups) >= GROUPS:
                break
            m = [lane for lane in range(WAVE) if same(lane, todo[0])]
            todo = [lane for lane in todo if lane not in m]
            if len(m) > 1:
                solo -= set(m)
                groups.append(len(m))
    return run, groups, len(solo)


def pose_plans(c, b):
    ok = np.zeros(-(-c.P // WAVE) * WAVE, bool)  # (the lanes past P are not live)
    j0 = np.zeros((len(ok), c.n_out), np.int64)
    with np.errstate(invalid="ignore"):
        _b, idx, cell, _w, _dw = list(SR._terms(c.grid, c.points, c.rot, c.trans, np.float64))[b]
    ok[idx], j0[idx] = True, cell
    return [wave_plan(ok[s:s + WAVE], j0[s:s + WAVE]) for s in range(0, len(ok), WAVE)]


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_wave_patterns_reach_the_combine_s_branches(n_in, n_out):
    """(CPU)  The table of the module docstring, rebuilt from the reference's cell choice under the identity pose."""
    c = pattern_case(n_in, n_out)
    assert c.P == 12 * WAVE + 20 and c.P % WAVE == 20 and c.P > 3 * 256  # (four workgroups, the last one partial)
    plans = pose_plans(c, 0)
    for w, plan in enumerate(plans):
        print(f"({n_in}, {n_out}) wave {w}: {plan}")
    assert plans == WAVE_PLAN
    # the cells are the ones asked for, the rejected lanes are rejected by both poses and carry NaN tangents
    with np.errstate(invalid="ignore"):
        _b, idx, j0, _w, _dw = next(iter(SR._terms(c.grid, c.points, c.rot, c.trans, np.float64)))
    want = [p for p, cell in enumerate(c.lanes) if not isinstance(cell, str)]
    assert np.array_equal(idx, want) and np.array_equal(j0, [c.lanes[p] for p in want])
    assert np.array_equal(np.nonzero(c.rejected)[0], [p for p, cell in enumerate(c.lanes) if isinstance(cell, str)])
    assert np.all(np.isnan(c.t["points"][:, c.rejected])) and np.all(np.isnan(c.t["point_weight"][:, c.rejected]))
    assert (j0[:, 0] == -1).sum() == 32 and (j0[:, -1] == 8).sum() == 32
    # pose 1 is generic, and no pattern survives the permutation: no wave of the permuted cloud searches
    print(f"({n_in}, {n_out}) pose 1: {pose_plans(c, 1)}")
    p = SimpleNamespace(**{**vars(c), "points": c.points[c.perm]})
    assert all(run < MIN_RUN and not groups for run, groups, _solo in pose_plans(p, 0))
    # every plane of the reference holds deposits, and every cell of the budget is positive
    assert np.all(c.A > 0) and c.n[..., 0].max() >= 64


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("order", ["as built", "permuted"])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_wave_patterns_deposit_by_deposit(dev, n_in, n_out, algo, order, npdt, tdt):
    c = pattern_case(n_in, n_out)
    out = device_jvp(c, c.t, KINDS, c.B, tdt, dev, algo, order=c.perm if order == "permuted" else None)
    assert tuple(out.shape) == c.grid + (c.K, c.B) and out.dtype == tdt
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out_dot"
    what = f"({n_in}, {n_out}) {algo} {order} {np.dtype(npdt).name}"
    if npdt == np.float64:
        eps = float(np.finfo(np.float64).eps)
        bound = (c.n[..., None, :] + 16) * eps * c.A
        ratio = np.abs(got - c.ref) / bound
        worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{what}: max |got - ref64| / ((n_c + 16) eps A_c) = {ratio.max():.3e} at {worst}")
        assert ratio.max() <= 1, f"{what}: cell, k, b = {worst}: |got - ref64| = {abs(got[worst] - c.ref[worst]):.3e}" \
            f" > {bound[worst]:.3e} ({c.n[worst[:-2] + worst[-1:]]} deposits, A = {c.A[worst]:.3e}); " \
            f"{int((ratio > 1).sum())} cells over the bound"
    else:
        check_planes_fp32(got, c.ref, RHO[("waves", n_in, n_out)], what)


# ------------------------------------------------------------------ 1b the hard inputs
@functools.lru_cache(maxsize=None)
def hard_tangents(name):
    h = smooth_input(name)
    t = make_tangents(np.random.default_rng(4200 + len(name) + h.n_in), 2, h.B, h.P, h.n_in, h.n_out)
    t["points"][:, -N_BAD:] = np.nan
    t["point_weight"][:, -N_BAD:] = np.nan
    return freeze_all(t)


def hard_case(name):
    h, s = smooth_input(name), smooth_data(name)
    return SimpleNamespace(grid=h.grid, points=h.points, rot=h.rot, trans=h.trans, ow=s.ow, pw=s.pw, P=h.P, B=h.B)


@functools.lru_cache(maxsize=None)
def hard_reference(name, tangents, dtype=np.float64):
    """grid + (2, 3); the planes of the first pose alone are [..., :1]"""
    out = reference(hard_case(name), hard_tangents(name), TANGENT_SETS[tangents], 3, dtype)
    assert np.all(np.isfinite(out))
    return frozen(out)


def measured_rho(key):
    if key[0] == "waves":
        c = pattern_case(*key[1:])
        ref32 = reference(c, c.t, KINDS, c.B, np.float32).astype(np.float64)
        return float(plane_ratios(ref32, c.ref).max())
    name, tangents = key
    return float(plane_ratios(hard_reference(name, tangents, np.float32).astype(np.float64),
                              hard_reference(name, tangents)).max())


RHO_KEYS = [("waves",) + p for p in PAIRS] + [(name, t) for name in INPUTS for t in TANGENT_SETS]


@pytest.mark.parametrize("key", RHO_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_recorded_rho_is_the_reference_s(key):
    """RHO against a fresh measurement on the CPU reference (deterministic): within 1 %."""
    rho = measured_rho(key)
    print(f"rho {key}: {rho:.4e}")
    assert key in RHO, f"{key}: measured {rho:.4e}, nothing recorded"
    assert abs(RHO[key] - rho) <= 0.01 * rho, f"{key}: recorded {RHO[key]:.4e}, measured {rho:.4e}"


@pytest.mark.parametrize("name", INPUTS)
def test_far_cells_hold_the_background_tangent_in_the_reference(name):
    """(CPU)  Where no point reaches, the fp64 reference is background_dot[k, b] exactly, and it is not everywhere."""
    far, t = far_cells(name), hard_tangents(name)
    for tangents in TANGENT_SETS:
        ref = hard_reference(name, tangents)
        want = np.broadcast_to(t["background"] if tangents == "all" else 0.0, ref.shape)
        mask = np.broadcast_to(far[..., None, :], ref.shape)
        assert np.array_equal(ref[mask], want[mask])
        assert not np.array_equal(ref, want)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("tangents", list(TANGENT_SETS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", INPUTS)
def test_hard_inputs_plane_by_plane(dev, name, algo, B, tangents, npdt, tdt):
    c, t, kinds = hard_case(name), hard_tangents(name), TANGENT_SETS[tangents]
    ref64 = hard_reference(name, tangents)[..., :B]
    out = device_jvp(c, t, kinds, B, tdt, dev, algo)
    assert tuple(out.shape) == c.grid + (2, B) and out.dtype == tdt
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), "non-finite out_dot: a NaN / Inf point or its NaN tangent was used"
    what = f"{name} {algo} B={B} {tangents} {np.dtype(npdt).name}"
    if npdt == np.float64:
        check_planes_fp64(out, ref64, what)
    else:
        check_planes_fp32(got, ref64, RHO[(name, tangents)], what)
    # cells nothing reaches hold the background tangent exactly (the tiled flush skips cells whose sum is 0)
    far = np.broadcast_to(far_cells(name)[..., None, :B], got.shape)
    want = np.broadcast_to((t["background"][:, :B] if tangents == "all" else np.zeros((2, B))).astype(npdt), got.shape)
    bad = far & (out.cpu().numpy() != want)
    assert far.any() and not bad.any(), f"{what}: {int(bad.sum())} of {int(far.sum())} far cells are not " \
        f"background_dot; first {tuple(int(v) for v in np.argwhere(bad)[0])}"
    # ... and the call without the five NaN / Inf points
    clean = device_jvp(c, t, kinds, B, tdt, dev, algo, keep=slice(0, c.P - N_BAD))
    assert_close(out, clean.cpu().numpy(), jvp_tol(npdt), f"{what}: with and without the five")


# ------------------------------------------------------------------ 1c key bits and small grids
@functools.lru_cache(maxsize=None)
def edge_jvp(n_in, grid):
    c = edge_case(n_in, grid)
    t = make_tangents(np.random.default_rng(4300 + n_in + sum(grid)), 3, c.B, c.P, n_in, len(grid))
    t["points"][:, -6:] = np.nan  # the six points no pose accepts
    t["point_weight"][:, -6:] = np.nan
    ref = reference(c, freeze_all(t), KINDS, c.B)
    assert np.all(np.isfinite(ref))
    return t, frozen(ref)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("n_in,n_out,grid", EDGE_CASES)
def test_key_bit_and_small_grid_edges(dev, n_in, n_out, grid, npdt, tdt):
    c = edge_case(n_in, grid)
    t, ref = edge_jvp(n_in, grid)
    tiled = device_jvp(c, t, KINDS, c.B, tdt, dev, "tiled")
    atomic = device_jvp(c, t, KINDS, c.B, tdt, dev, "atomic")
    assert tuple(tiled.shape) == grid + (3, c.B)
    assert bool(torch.isfinite(tiled).all()) and bool(torch.isfinite(atomic).all())
    for k in range(3):
        for b in range(c.B):  # plane by plane: a plane must not hide in another's norm
            e = ref[..., k, b].astype(npdt)
            assert_close(tiled[..., k, b], e, jvp_tol(npdt), f"{grid} tiled, plane ({k}, {b})")
            assert_close(atomic[..., k, b], e, jvp_tol(npdt), f"{grid} atomic, plane ({k}, {b})")
            assert_close(tiled[..., k, b], atomic[..., k, b].cpu().numpy(), jvp_tol(npdt),
                         f"{grid} tiled vs atomic, plane ({k}, {b})")
