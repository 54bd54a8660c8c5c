"""The fp32 sum contract (include/dpr.h, PRECISION OF THE FIXED-POINT SUMS) in the four op families that choose the
fixed-point scale and the 2^10 range guard with code of their own: the TILED JVP (scope: the (pose, tangent), from
the per-record bound |a| + sum |b_n|), the TILED channel forward (scope: the channel of a pose), the CHUNKED per-pose
clouds (key per pose, scale per (pose, tile, slice)) and the TILED sampling pullback (one single-pose raster per
column of ds_dvalues) -- each with the ATOMIC path under the same bound.

Inputs: uniform clouds on grids of several tiles with no tile split into parts (so the fixed-point sums are exact
wherever the guard does not trip), three poses (pose 0 the identity), eight points far outside every grid, all
values rounded to fp32 once and used for both dtypes.  Weight fields, applied to whatever plays the weight:
`narrow` 2^U(0, 9) signed (fixed point kept), `wide` 2^U(-40, 0) signed, `slabs` five regions 2^0 .. 2^-40 along
axis 0 (whole tiles hold only light points), `tiny` 2^-40 U(1, 2) (the scale must follow the scope's maximum), and
exact zeros on a tenth of the points of `narrow` and `wide`.  `wide` always comes BEFORE `tiny` in the order of
channels, tangents, poses and columns, so that a key left over from the previous scope meets the scope it would
hurt most.  (The keys merge by maximum: as the kernels stand, a leftover key can only trip the next scope's guard,
which costs that scope its exact sums, not its precision -- the per-cell bound cannot see that, the bit-equality
checks see it only through rounding ties.)

The per-cell bound (fp32; no cell is skipped): |got - ref64|(cell) <= m * S(cell) on every image-shaped plane.
ref64 is the fp64 oracle on the fp32-rounded inputs (for the JVP: tests/test_jvp_abi.py's restatement with the fp32
cell choice); S(cell) is the sum over the accepted points that touch the cell -- by the fp32 cell choice, any of
the 2^N corners -- of the point's magnitude |out_weight * weight| (JVP: |a| + sum |b_n| in fp64), so a cell reached
only by light points is held to ITS OWN scale; cells with S = 0 equal the background bit for bit.
m = max(4 rho, 8 eps32): rho is the reference's own fp32 rounding at this input, the maximum over the cells with
S > 0 of |ref32 - ref64| / S with ref32 the fp32 oracle (JVP: the restatement with value_dtype = fp32), measured on
the CPU -- `python -m tests.test_families_precision_gpu` prints the table below from `measure_rho`; the factor 4
and the floor are tests/test_families_hard_gpu.py's (the device sums in another order but in at least the oracle's
precision).  The cases with a non-zero background use `narrow` weights only (a background of order 1 rounds the
cell to eps32 of ITSELF, which only cells with S of order 1 can absorb) and have a rho of their own.

    family / case / input            rho
    jvp / a / W3                     1.412e-07
    jvp / b / W3                     1.448e-07
    jvp / c_wide / W3                1.888e-07
    jvp / c_narrow / W3              1.309e-07
    jvp / bg / W3                    1.757e-07
    jvp / a / W2_32                  1.770e-07
    jvp / b / W2_32                  2.434e-07
    jvp / c_wide / W2_32             2.230e-07
    jvp / c_narrow / W2_32           1.415e-07
    jvp / bg / W2_32                 1.477e-07
    jvp / a / W2_22                  1.633e-07
    channels / wide / W3             1.079e-05
    channels / bg / W3               9.633e-06
    channels / wide / W2_32          1.034e-05
    channels / bg / W2_32            1.017e-05
    clouds / perpose / C2 / 1500     4.935e-06
    clouds / shared / C2 / 1500      4.635e-06
    clouds / bg / C2 / 1500          4.880e-06
    clouds / perpose / C2 / 20000    5.301e-06
    clouds / shared / C2 / 20000     5.298e-06
    clouds / bg / C2 / 20000         5.315e-06
    clouds / perpose / C3 / 1500     3.541e-06
    clouds / shared / C3 / 1500      3.562e-06
    clouds / bg / C3 / 1500          3.566e-06
    clouds / perpose / C3 / 20000    3.723e-06
    clouds / shared / C3 / 20000     3.730e-06
    clouds / bg / C3 / 20000         3.746e-06
    sample / W3                      8.858e-06
    sample / W2_32                   8.504e-06
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dpr_amd
from oracle import oracle
from tests import data as D
from tests.test_channels_gpu import _bit_equal_or_rounding, assert_close, plane, single as single_channel, tol
from tests.test_clouds_gpu import clouds as make_clouds, on as clouds_on, oracle_forward
from tests.test_families_hard_gpu import TILE, channel_problem, check_sample_pullback, poses, r32, tile_counts, to
from tests.test_jvp_abi import cell_choice, footprint_sum, jvp_reference, jvp_terms
from tests.test_jvp_gpu import tol as jvp_tol
from tests.test_parity_gpu import _weight_field

gpu = pytest.mark.gpu

DTYPES = [(np.float64, torch.float64), (np.float32, torch.float32)]
EPS32 = float(np.finfo(np.float32).eps)
# name: n_in, n_out, grid, points, seed.  The heaviest tile of the identity pose holds ~4000 (W3) / ~1950 (W2) records, just
# under the caps below; the seeds are ones whose poses 1 and 2 stay under them too (test_no_tile_is_split).
SPEC = {
    "W3": (3, 3, (96, 40, 24), 40_000, 154),
    "W2_32": (3, 2, (100, 70), 12_000, 44),
    "W2_22": (2, 2, (100, 70), 12_000, 13),
}
CAP = {3: 4096, 2: 2048}  # records per tile below which no path splits a tile (make_plan in csrc/dpr_tiled_plan.hip)
FAR = 8  # points far outside every grid, appended to every input
CLOUD_GRIDS = {"C2": (64, 64), "C3": (40, 33, 20)}
CLOUD_P = (1500, 20_000)  # one slice per (pose, tile) / several slices (test_chunked_tiles_and_slices)
M_FACTOR = 4.0
RHO = {
    ("jvp", "a", "W3"): 1.412e-07,
    ("jvp", "b", "W3"): 1.448e-07,
    ("jvp", "c_wide", "W3"): 1.888e-07,
    ("jvp", "c_narrow", "W3"): 1.309e-07,
    ("jvp", "bg", "W3"): 1.757e-07,
    ("jvp", "a", "W2_32"): 1.770e-07,
    ("jvp", "b", "W2_32"): 2.434e-07,
    ("jvp", "c_wide", "W2_32"): 2.230e-07,
    ("jvp", "c_narrow", "W2_32"): 1.415e-07,
    ("jvp", "bg", "W2_32"): 1.477e-07,
    ("jvp", "a", "W2_22"): 1.633e-07,
    ("channels", "wide", "W3"): 1.079e-05,
    ("channels", "bg", "W3"): 9.633e-06,
    ("channels", "wide", "W2_32"): 1.034e-05,
    ("channels", "bg", "W2_32"): 1.017e-05,
    ("clouds", "perpose", "C2", 1500): 4.935e-06,
    ("clouds", "shared", "C2", 1500): 4.635e-06,
    ("clouds", "bg", "C2", 1500): 4.880e-06,
    ("clouds", "perpose", "C2", 20000): 5.301e-06,
    ("clouds", "shared", "C2", 20000): 5.298e-06,
    ("clouds", "bg", "C2", 20000): 5.315e-06,
    ("clouds", "perpose", "C3", 1500): 3.541e-06,
    ("clouds", "shared", "C3", 1500): 3.562e-06,
    ("clouds", "bg", "C3", 1500): 3.566e-06,
    ("clouds", "perpose", "C3", 20000): 3.723e-06,
    ("clouds", "shared", "C3", 20000): 3.730e-06,
    ("clouds", "bg", "C3", 20000): 3.746e-06,
    ("sample", "W3"): 8.858e-06,
    ("sample", "W2_32"): 8.504e-06,
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ inputs and weight fields
@functools.lru_cache(maxsize=None)
def wide_input(name):
    n_in, n_out, grid, P, seed = SPEC[name]
    d = D.make(n_points=4, n_in=n_in, n_out=n_out, batch=3, grid_n=grid, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    pts = rng.uniform(-0.95, 0.95, size=(P, n_in))
    far = 9.0 * rng.choice([-1.0, 1.0], size=(FAR, n_in))
    rot, trans = d.rotations.copy(), d.translations.copy()
    rot[0] = np.eye(n_out, n_in)
    trans[0] = 0.0
    return SimpleNamespace(name=name, n_in=n_in, n_out=n_out, grid=grid, P=P + FAR, B=3,
                           points=r32(np.concatenate([pts, far])), rot=r32(rot), trans=r32(trans))


def field(kind, rng, n, x01=None, zeros=False):
    """One weight field of the module docstring, (n,) rounded to fp32."""
    sign = np.ones(n)
    sign[rng.permutation(n)[: n // 2]] = -1.0
    if kind == "narrow":
        w = sign * 2.0 ** rng.uniform(0, 9, n)
    elif kind == "wide":
        w = sign * 2.0 ** rng.uniform(-40, 0, n)
    elif kind == "slabs":
        w = _weight_field("slabs", x01, rng).astype(np.float64)
    else:
        assert kind == "tiny"
        w = 2.0 ** -40 * rng.uniform(1, 2, n)
    if zeros:
        w[::10] = 0.0
    return r32(w)


def span(mag):
    """max / min of the non-zero magnitudes"""
    m = np.abs(np.asarray(mag, np.float64))
    m = m[m > 0]
    return float(m.max() / m.min())


@functools.lru_cache(maxsize=None)
def cells(name, b):
    h = wide_input(name)
    ok, ref0, _ = cell_choice(h.grid, h.points, h.rot[b], h.trans[b], np.float32)
    return ok, ref0


def accepted_by_all(h, n, skip_tenth=True):
    """the first n points that every pose of h accepts (not the ones the fields set to zero)"""
    ok = cells(h.name, 0)[0] & cells(h.name, 1)[0] & cells(h.name, 2)[0]
    if skip_tenth:
        ok[::10] = False
    return np.nonzero(ok)[0][:n]


# ------------------------------------------------------------------ the per-cell bound
def m_of(key):
    return max(M_FACTOR * RHO[key], 8 * EPS32)


def worst_ratio(x, ref64, S):
    pos = S > 0
    return float((np.abs(np.asarray(x, np.float64) - ref64)[pos] / S[pos]).max()) if pos.any() else 0.0


def bits_equal(a32, value):
    return bool(np.all(np.ascontiguousarray(a32).view(np.uint32) == np.float32(value).view(np.uint32)))


def sbound(got, ref64, S, bg, key, what):
    """|got - ref64| <= m * S on one plane of an fp32 result; the cells with S = 0 hold the background's bits."""
    g = got.detach().cpu().numpy()
    assert g.dtype == np.float32 and g.shape == S.shape, f"{what}: {g.dtype} {g.shape} != {S.shape}"
    assert np.all(np.isfinite(g)), f"{what}: non-finite cells"
    zero = S == 0
    assert bits_equal(g[zero], bg), f"{what}: {int((g[zero] != np.float32(bg)).sum())} untouched cells differ from " \
                                    f"the background"
    r, m = worst_ratio(g, ref64, S), m_of(key)
    print(f"{'/'.join(map(str, key))} {what}: max|got - ref64| / S = {r:.3e} (m = {m:.3e})")
    assert r <= m, f"{what}: max|got - ref64| / S = {r:.3e} > m = {m:.3e}"


def same_sets(got, ref32, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.isnan(ref32).any(), f"{what}: the reference has no NaN cell"
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(g), f(ref32)), f"{what}: {f.__name__} cells differ from the fp32 reference's"
    return np.isfinite(ref32)


def unchanged(got, clean, exact, what):
    if exact:
        assert torch.equal(got, clean), f"{what}: not bit-identical to the call without the non-finite values"
    else:
        assert_close(got, clean, 1e-6, what)


# ------------------------------------------------------------------ 1. JVP
JVP_CASES = [(n, c) for n in ("W3", "W2_32") for c in ("a", "b", "c_wide", "c_narrow", "bg")] + [("W2_22", "a")]
POSE_KINDS = ("rotation", "translation", "background", "out_weight")


@functools.lru_cache(maxsize=None)
def jvp_case(name, case):
    h = wide_input(name)
    rng = np.random.default_rng(SPEC[name][4] + 17 + sum(map(ord, case)))
    x01 = (h.points[:, 0] + 1) / 2
    f = lambda kind, **kw: field(kind, rng, h.P, x01, **kw)
    ow = r32(rng.uniform(0.5, 2.0, size=3))
    if case == "a":  # point_weight tangents; the deposit ow * point_weight_dot of a point of weight 0 must survive
        pw, tan = f("narrow", zeros=True), dict(point_weight=np.stack([f("wide", zeros=True), f("tiny"),
                                                                       f("narrow", zeros=True)]))
    elif case == "b":  # geometric tangents: a = 0, everything in b_n
        pw = None
        tan = dict(points=r32(np.stack([f("slabs")[:, None] * rng.normal(size=(h.P, h.n_in)),
                                        f("tiny")[:, None] * rng.normal(size=(h.P, h.n_in))])))
    elif case in ("c_wide", "c_narrow"):  # tangent 0: translation only, tangent 1: out_weight only
        pw = f("wide") if case == "c_wide" else f("narrow", zeros=True)
        td, owd = rng.normal(size=(2, 3, h.n_out)), rng.normal(size=(2, 3))
        td[1], owd[0] = 0.0, 0.0
        tan = dict(translation=r32(td), out_weight=r32(owd))
    elif case == "bg":  # a non-zero background tangent under narrow deposits
        pw, tan = f("narrow", zeros=True), dict(point_weight=np.stack([f("narrow"), f("narrow", zeros=True)]),
                                                background=r32(rng.normal(size=(2, 3))))
    else:  # "d": moderate magnitudes; the non-finite entries are put in by the test
        pw, tan = r32(rng.uniform(0.5, 2.0, size=h.P)), dict(point_weight=r32(rng.normal(size=(3, h.P))),
                                                             out_weight=r32(rng.normal(size=(3, 3))))
    K = len(next(iter(tan.values())))
    return SimpleNamespace(K=K, ow=ow, pw=pw, tan=tan,
                           bg=tan.get("background", np.zeros((K, 3))))


def jvp_ref(h, j, cell_dtype, value_dtype=np.float64, tan=None):
    with np.errstate(invalid="ignore", over="ignore"):
        return jvp_reference(h.grid, h.points, h.rot, h.trans, j.ow, j.pw, j.tan if tan is None else tan, j.K,
                             cell_dtype=cell_dtype, value_dtype=value_dtype)


@functools.lru_cache(maxsize=None)
def jvp_expected(name, case):
    """ref64 / ref32 (fp32 cells), S and the per-scope spans of the bound; `cells64`: the fp64 tests' reference"""
    h, j = wide_input(name), jvp_case(name, case)
    S, spans = np.zeros(h.grid + (j.K, 3)), np.zeros((j.K, 3))
    for b in range(3):
        ok, ref0, a, bn = jvp_terms(h.grid, h.points, h.rot, h.trans, j.ow, j.pw, j.tan, j.K, b, np.float32)
        bound = np.abs(a) + np.abs(bn).sum(-1)
        for k in range(j.K):
            S[..., k, b] = footprint_sum(h.grid, ok, ref0, bound[k])
            spans[k, b] = span(bound[k][ok])
    return SimpleNamespace(ref64=jvp_ref(h, j, np.float32), ref32=jvp_ref(h, j, np.float32, np.float32), S=S,
                           spans=spans, bg=j.bg)


@functools.lru_cache(maxsize=None)
def jvp_cells64(name, case):
    return jvp_ref(wide_input(name), jvp_case(name, case), np.float64)


def run_jvp(h, j, tdt, dev, algo, single, tan=None):
    """out_dot as (grid..., K, poses)"""
    t = lambda a: None if a is None else to(a, tdt, dev)
    kw = {}
    for kind, v in (j.tan if tan is None else tan).items():
        kw[kind + "_dot"] = t(v[:, 0] if single and kind in POSE_KINDS else v)
    s = (lambda a: a[0]) if single else (lambda a: a)
    out = dpr_amd.raster_jvp(h.grid, t(h.points), t(s(h.rot)), t(s(h.trans)), None, t(j.ow[:1] if single else j.ow),
                             t(j.pw), **kw, tangents=j.K, algo=algo)
    assert tuple(out.shape) == tuple(h.grid) + (j.K,) + (() if single else (3,))
    return out.unsqueeze(-1) if single else out


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name,case", JVP_CASES)
def test_jvp(dev, name, case, algo, npdt, tdt):
    h, j, e = wide_input(name), jvp_case(name, case), jvp_expected(name, case)
    ref = e.ref64 if npdt == np.float32 else jvp_cells64(name, case)
    for single in (True, False):
        out = run_jvp(h, j, tdt, dev, algo, single)
        assert bool(torch.isfinite(out).all()), "non-finite out_dot"
        for k in range(j.K):
            for i, b in enumerate(poses(single)):
                what = f"{algo} single={single} out_dot[.., {k}, {b}]"
                assert_close(out[..., k, i].double(), ref[..., k, b], jvp_tol(npdt), what)
                if npdt == np.float32:
                    sbound(out[..., k, i], e.ref64[..., k, b], e.S[..., k, b], e.bg[k, b], ("jvp", case, name), what)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name", ["W3", "W2_32"])
def test_jvp_non_finite_tangents_stay_in_their_planes(dev, name, algo, npdt, tdt):
    """NaN, +Inf and -Inf in point_weight_dot[1] on points every pose accepts; then a NaN in out_weight_dot[1, 1].
    The other (tangent, pose) planes equal the call with those entries set to 0; the affected planes have the
    restatement's NaN / +Inf / -Inf cells and stay right elsewhere."""
    h, j = wide_input(name), jvp_case(name, "d")
    exact = algo == "tiled" and h.n_out == 3 and npdt == np.float32
    i_nan, i_pinf, i_ninf = accepted_by_all(h, 3, skip_tenth=False)
    for where in ("point_weight", "out_weight"):
        clean_tan = {k: v.copy() for k, v in j.tan.items()}
        if where == "point_weight":
            clean_tan["point_weight"][1, [i_nan, i_pinf, i_ninf]] = 0.0
            bad_tan = {k: v.copy() for k, v in clean_tan.items()}
            bad_tan["point_weight"][1, [i_nan, i_pinf, i_ninf]] = [np.nan, np.inf, -np.inf]
            affected = lambda k, b: k == 1
        else:
            clean_tan["out_weight"][1, 1] = 0.0
            bad_tan = {k: v.copy() for k, v in clean_tan.items()}
            bad_tan["out_weight"][1, 1] = np.nan
            affected = lambda k, b: (k, b) == (1, 1)
        ref32 = jvp_ref(h, j, npdt, np.float32, tan=bad_tan)
        ref = jvp_ref(h, j, npdt, tan=clean_tan)
        for single in (True, False) if where == "point_weight" else (False,):
            out = run_jvp(h, j, tdt, dev, algo, single, tan=bad_tan)
            clean = run_jvp(h, j, tdt, dev, algo, single, tan=clean_tan)
            for k in range(j.K):
                for i, b in enumerate(poses(single)):
                    what = f"{where} {algo} single={single} out_dot[.., {k}, {b}]"
                    if affected(k, b):
                        fin = same_sets(out[..., k, i], ref32[..., k, b], what)
                        assert_close(out[..., k, i].cpu().numpy()[fin], ref[..., k, b][fin], jvp_tol(npdt), what)
                    else:
                        unchanged(out[..., k, i], clean[..., k, i], exact, what)
                        assert_close(out[..., k, i].double(), ref[..., k, b], jvp_tol(npdt), what)


# ------------------------------------------------------------------ 2. channels
@functools.lru_cache(maxsize=None)
def channel_case(name, case):
    h = wide_input(name)
    rng = np.random.default_rng(SPEC[name][4] + 100 + sum(map(ord, case)))
    x01 = (h.points[:, 0] + 1) / 2
    f = lambda kind, **kw: field(kind, rng, h.P, x01, **kw)
    if case == "wide":
        pw, bg = np.stack([f("wide", zeros=True), f("tiny"), f("narrow", zeros=True), f("slabs")], 1), np.zeros((3, 4))
    else:  # "bg": a non-zero background under narrow weights
        pw, bg = np.stack([f("narrow", zeros=True), f("narrow")], 1), r32(rng.uniform(-1, 1, size=(3, 2)))
    return SimpleNamespace(pw=pw, bg=bg, ow=r32(rng.uniform(0.5, 2.0, size=3)), C=pw.shape[1])


def channel_refs(h, ch, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([oracle.raster(h.grid, h.points, h.rot, h.trans, ch.bg[:, c], ch.ow, ch.pw[:, c], dtype=dtype)
                         for c in range(ch.C)], axis=h.n_out)


@functools.lru_cache(maxsize=None)
def channel_expected(name, case):
    h, ch = wide_input(name), channel_case(name, case)
    S, spans = np.zeros(h.grid + (ch.C, 3)), np.zeros((ch.C, 3))
    for b in range(3):
        ok, ref0 = cells(name, b)
        for c in range(ch.C):
            S[..., c, b] = footprint_sum(h.grid, ok, ref0, np.abs(ch.ow[b] * ch.pw[:, c]))
            spans[c, b] = span(ch.pw[ok, c])
    return SimpleNamespace(ref64=channel_refs(h, ch, np.float64), ref32=channel_refs(h, ch, np.float32), S=S,
                           spans=spans)


def run_channels(h, ch, tdt, dev, algo, single, **over):
    """out as (grid..., C, poses) and the problem dict"""
    p = dict(channel_problem(h, ch, ch.C, tdt, dev, single), **over)
    out = dpr_amd.raster_channels(h.grid, p["points"], p["rot"], p["trans"], p["pw"], p["bg"], p["ow"], algo=algo)
    assert tuple(out.shape) == tuple(h.grid) + (ch.C,) + (() if single else (3,))
    return (out.unsqueeze(-1) if single else out), p


def check_channel_planes(out, h, ch, e, channels, single, npdt, key, what):
    ref = e.ref64 if npdt == np.float64 else e.ref32
    for c in channels:
        for i, b in enumerate(poses(single)):
            w = f"{what} single={single} out[.., {c}, {b}]"
            got = plane(out, c, h.n_out)[..., i]
            assert_close(got, ref[..., c, b], tol(npdt, "out"), w)
            if npdt == np.float32:
                sbound(got, e.ref64[..., c, b], e.S[..., c, b], ch.bg[b, c], key, w)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("case", ["wide", "bg"])
@pytest.mark.parametrize("name", ["W3", "W2_32"])
def test_channels(dev, name, case, algo, npdt, tdt):
    h, ch, e = wide_input(name), channel_case(name, case), channel_expected(name, case)
    for single in (True, False):
        out, _ = run_channels(h, ch, tdt, dev, algo, single)
        check_channel_planes(out, h, ch, e, range(ch.C), single, npdt, ("channels", case, name), algo)


@gpu
def test_channels_tiled_fp32_tiny_and_narrow_planes_are_exact(dev):
    """W3, fp32: the `tiny` plane after the `wide` one and the `narrow` plane keep their fixed-point sums -- the same
    bits under a permutation of the points (no tile is split), and the single-channel call's."""
    h, ch = wide_input("W3"), channel_case("W3", "wide")
    perm = torch.randperm(h.P, generator=torch.Generator().manual_seed(1)).to(dev)
    for single in (True, False):
        out, p = run_channels(h, ch, torch.float32, dev, "tiled", single)
        outp, _ = run_channels(h, ch, torch.float32, dev, "tiled", single, points=p["points"][perm].contiguous(),
                               pw=p["pw"][perm].contiguous())
        for c in (1, 2):
            assert torch.equal(plane(out, c, 3), plane(outp, c, 3)), f"single={single} plane {c}: order-dependent"
            if single:
                ref, rerun = single_channel(p, c, "tiled"), single_channel(p, c, "tiled")
                _bit_equal_or_rounding(plane(out, c, 3)[..., 0], ref, rerun, f"plane {c}")


@gpu
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name", ["W3", "W2_32"])
def test_channels_non_finite_weights_stay_in_their_channel(dev, name, algo):
    """NaN, +Inf and -Inf in channel 0 of three points: channels 1-3 are what they were, channel 0 has the fp32
    oracle's NaN / +Inf / -Inf cells and stays right elsewhere."""
    h, ch, e = wide_input(name), channel_case(name, "wide"), channel_expected(name, "wide")
    bad = SimpleNamespace(pw=ch.pw.copy(), bg=ch.bg, ow=ch.ow, C=ch.C)
    bad.pw[accepted_by_all(h, 3), 0] = [np.nan, np.inf, -np.inf]
    ref32 = channel_refs(h, bad, np.float32)
    for single in (True, False):
        out, _ = run_channels(h, bad, torch.float32, dev, algo, single)
        clean, _ = run_channels(h, ch, torch.float32, dev, algo, single)
        check_channel_planes(out, h, ch, e, (1, 2, 3), single, np.float32, ("channels", "wide", name), algo)
        for c in (1, 2, 3):
            exact = algo == "tiled" and h.n_out == 3 and c in (1, 2)
            unchanged(plane(out, c, h.n_out), plane(clean, c, h.n_out), exact, f"single={single} plane {c}")
        for i, b in enumerate(poses(single)):
            what = f"{algo} single={single} out[.., 0, {b}]"
            got = plane(out, 0, h.n_out)[..., i].cpu().numpy()
            fin = same_sets(got, ref32[..., 0, b], what)
            assert_close(got[fin], ref32[..., 0, b][fin], tol(np.float32, "out"), what)


# ------------------------------------------------------------------ 3. per-pose clouds, CHUNKED
CLOUD_CASES = [(g, P, c) for g in CLOUD_GRIDS for P in CLOUD_P for c in ("perpose", "shared", "bg")]


@functools.lru_cache(maxsize=None)
def cloud_case(gname, P, case):
    """The clouds of test_chunked_tiles_and_slices (pose 0 the identity with points on cell faces, a fiftieth of each
    cloud outside the grid) with point_weight (B, P): pose 0 `wide` under out_weight 2^12, pose 1 `tiny`, pose 2
    `narrow`; `shared`: one (P,) `slabs` field for all poses; `bg`: `narrow` on a non-zero background."""
    grid = CLOUD_GRIDS[gname]
    c = make_clouds(3, len(grid), B=3, P=P, grid=grid, seed=P + len(grid), pad=False)
    for k in ("points", "rot", "trans", "ds"):
        c[k] = r32(c[k])
    rng = np.random.default_rng(P + len(grid) + sum(map(ord, case)))
    f = lambda kind, **kw: field(kind, rng, P, (np.clip(c["points"][0][:, 0], -1, 1) + 1) / 2, **kw)
    ow = r32(rng.uniform(0.5, 2.0, size=3))
    c["bg"] = np.zeros(3)
    c["shared"] = case == "shared"
    if case == "perpose":
        c["pw"] = np.stack([f("wide", zeros=True), f("tiny"), f("narrow", zeros=True)])
        ow[0] = 4096.0
    elif case == "shared":
        c["pw"] = np.broadcast_to(f("slabs"), (3, P)).copy()
    else:
        c["pw"] = np.stack([f("narrow", zeros=True), f("narrow"), f("narrow")])
        c["bg"] = r32(rng.uniform(-1, 1, size=3))
    c["ow"] = ow
    return c


def cloud_refs(c, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([oracle_forward(c, dtype, b) for b in range(3)], axis=-1)


def cloud_cells(c, b):
    ok, ref0, _ = cell_choice(c["grid"], c["points"][b], c["rot"][b], c["trans"][b], np.float32)
    return ok, ref0


@functools.lru_cache(maxsize=None)
def cloud_expected(gname, P, case):
    c = cloud_case(gname, P, case)
    S, spans = np.zeros(c["grid"] + (3,)), np.zeros(3)
    for b in range(3):
        ok, ref0 = cloud_cells(c, b)
        S[..., b] = footprint_sum(c["grid"], ok, ref0, np.abs(c["ow"][b] * c["pw"][b]))
        spans[b] = span(c["pw"][b])  # (the key of a pose is taken over its whole cloud)
    return SimpleNamespace(ref64=cloud_refs(c, np.float64), ref32=cloud_refs(c, np.float32), S=S, spans=spans)


def run_clouds(c, tdt, dev, **over):
    t = dict(clouds_on(dev, tdt, c), **over)
    pw = t["pw"][0].contiguous() if c["shared"] else t["pw"]
    out = dpr_amd.raster_clouds(c["grid"], t["points"], t["rot"], t["trans"], t["bg"], t["ow"], pw, algo="chunked")
    assert tuple(out.shape) == tuple(c["grid"]) + (3,)
    return out, t


def check_cloud_planes(out, c, e, planes, npdt, key):
    ref = e.ref64 if npdt == np.float64 else e.ref32
    for b in planes:
        assert_close(out[..., b], ref[..., b], tol(npdt, "out"), f"out[.., {b}]")
        if npdt == np.float32:
            sbound(out[..., b], e.ref64[..., b], e.S[..., b], c["bg"][b], key, f"out[.., {b}]")


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("gname,P,case", CLOUD_CASES)
def test_clouds_chunked(dev, gname, P, case, npdt, tdt):
    c, e = cloud_case(gname, P, case), cloud_expected(gname, P, case)
    out, _ = run_clouds(c, tdt, dev)
    check_cloud_planes(out, c, e, range(3), npdt, ("clouds", case, gname, P))


@gpu
@pytest.mark.parametrize("gname", list(CLOUD_GRIDS))
def test_clouds_chunked_fp32_one_slice_tiny_and_narrow_planes_are_exact(dev, gname):
    """test_chunked_fp32_one_slice_is_exact_and_order_independent with these weights: the `tiny` and `narrow` poses
    after the `wide` one keep their fixed-point sums, the same bits for any order of their clouds."""
    c = cloud_case(gname, CLOUD_P[0], "perpose")
    out, t = run_clouds(c, torch.float32, dev)
    perm = torch.stack([torch.randperm(c["P"], generator=torch.Generator().manual_seed(b)) for b in range(3)]).to(dev)
    pts = torch.gather(t["points"], 1, perm[..., None].expand(-1, -1, 3)).contiguous()
    outp, _ = run_clouds(c, torch.float32, dev, points=pts, pw=torch.gather(t["pw"], 1, perm).contiguous())
    for b in (1, 2):
        assert torch.equal(out[..., b], outp[..., b]), f"plane {b}: order-dependent"


@gpu
@pytest.mark.parametrize("P", CLOUD_P)
@pytest.mark.parametrize("gname", list(CLOUD_GRIDS))
def test_clouds_chunked_non_finite_weights_stay_in_their_pose(dev, gname, P):
    """Cloud 0: NaN and +Inf on accepted points, -Inf on a point outside the grid (it changes the path its pose
    takes, nothing else).  Planes 1-2 are what they were; plane 0 has the fp32 oracle's non-finite cells."""
    c, e = cloud_case(gname, P, "perpose"), cloud_expected(gname, P, "perpose")
    ok = cloud_cells(c, 0)[0]
    inside, outside = np.nonzero(ok)[0], np.nonzero(~ok)[0]
    bad = dict(c, pw=c["pw"].copy())
    bad["pw"][0, inside[[1, 2]]] = [np.nan, np.inf]
    bad["pw"][0, outside[0]] = -np.inf
    ref32 = cloud_refs(bad, np.float32)
    assert not np.isneginf(ref32).any()
    out, _ = run_clouds(bad, torch.float32, dev)
    clean, _ = run_clouds(c, torch.float32, dev)
    check_cloud_planes(out, c, e, (1, 2), np.float32, ("clouds", "perpose", gname, P))
    for b in (1, 2):
        unchanged(out[..., b], clean[..., b], P == CLOUD_P[0], f"plane {b}")
    got = out[..., 0].cpu().numpy()
    fin = same_sets(got, ref32[..., 0], "out[.., 0]")
    assert_close(got[fin], ref32[..., 0][fin], tol(np.float32, "out"), "out[.., 0]")


# ------------------------------------------------------------------ 4. sampling pullback
@functools.lru_cache(maxsize=None)
def sample_case(name):
    h = wide_input(name)
    rng = np.random.default_rng(SPEC[name][4] + 200)
    f = lambda kind, **kw: field(kind, rng, h.P, **kw)
    return SimpleNamespace(image=r32(rng.normal(size=h.grid + (3,))),
                           dv=np.stack([f("wide", zeros=True), f("tiny"), f("narrow", zeros=True)], 1))


def sample_refs(h, dv, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([oracle.raster(h.grid, h.points, h.rot[b:b + 1], h.trans[b:b + 1], None, None, dv[:, b],
                                       dtype=dtype)[..., 0] for b in range(3)], axis=-1)


@functools.lru_cache(maxsize=None)
def sample_expected(name):
    h, s = wide_input(name), sample_case(name)
    S, spans = np.zeros(h.grid + (3,)), np.zeros(3)
    for b in range(3):
        ok, ref0 = cells(name, b)
        S[..., b] = footprint_sum(h.grid, ok, ref0, np.abs(s.dv[:, b]))
        spans[b] = span(s.dv[ok, b])
    return SimpleNamespace(ref64=sample_refs(h, s.dv, np.float64), ref32=sample_refs(h, s.dv, np.float32), S=S,
                           spans=spans)


def run_sample_pullback(h, s, dv, tdt, dev, algo, single):
    t = lambda a: to(a, tdt, dev)
    img = dpr_amd.to_grid_layout(t(s.image))
    if single:
        pb = dpr_amd.sample_pullback_(t(dv[:, 0]), img[..., 0], t(h.points), t(h.rot[0]), t(h.trans[0]), algo=algo)
    else:
        pb = dpr_amd.sample_pullback_(t(dv), img, t(h.points), t(h.rot), t(h.trans), algo=algo)
    torch.cuda.synchronize()
    return pb, (pb.image.unsqueeze(-1) if single else pb.image)


@gpu
@pytest.mark.parametrize("npdt,tdt", DTYPES)
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name", ["W3", "W2_32"])
def test_sample_pullback(dev, name, algo, npdt, tdt):
    h, s, e = wide_input(name), sample_case(name), sample_expected(name)
    for single in (True, False):
        sel = list(poses(single))
        pb, image = run_sample_pullback(h, s, s.dv, tdt, dev, algo, single)
        check_sample_pullback(pb, h.grid, h.points, h.rot[sel], h.trans[sel], s.image[..., sel], s.dv[:, sel], npdt,
                              single)
        if npdt == np.float32:
            for i, b in enumerate(sel):
                sbound(image[..., i], e.ref64[..., b], e.S[..., b], 0.0, ("sample", name),
                       f"{algo} single={single} ds_dimage[.., {b}]")


@gpu
@pytest.mark.parametrize("algo", ["tiled", "atomic"])
@pytest.mark.parametrize("name", ["W3", "W2_32"])
def test_sample_pullback_nan_sensitivity_stays_in_its_plane(dev, name, algo):
    """A NaN in column 0 of ds_dvalues at a point every pose accepts and at a point every pose rejects: it shows in
    plane 0 of ds_dimage at the oracle's cells; planes 1-2 and the pose gradients of poses 1-2 are what they were."""
    h, s, e = wide_input(name), sample_case(name), sample_expected(name)
    dv = s.dv.copy()
    dv[[accepted_by_all(h, 1)[0], h.P - 1], 0] = np.nan
    assert not cells(name, 0)[0][h.P - 1]
    ref32 = sample_refs(h, dv, np.float32)
    for single in (True, False):
        pb, image = run_sample_pullback(h, s, dv, torch.float32, dev, algo, single)
        fin = same_sets(image[..., 0], ref32[..., 0], f"{algo} single={single} ds_dimage[.., 0]")
        assert_close(image[..., 0].cpu().numpy()[fin], ref32[..., 0][fin], tol(np.float32, "out"), "ds_dimage[.., 0]")
        if single:
            continue
        _, clean = run_sample_pullback(h, s, s.dv, torch.float32, dev, algo, single)
        for b in (1, 2):
            what = f"{algo} ds_dimage[.., {b}]"
            unchanged(image[..., b], clean[..., b], algo == "tiled" and h.n_out == 3, what)
            sbound(image[..., b], e.ref64[..., b], e.S[..., b], 0.0, ("sample", name), what)
            r = oracle.raster_pullback(s.image[..., b:b + 1], h.points, h.rot[b:b + 1], h.trans[b:b + 1], np.ones(1),
                                       dv[:, b], dtype=np.float32)
            for got, want, w in ((pb.rotation[b], r.rotation[0], "ds_drotation"),
                                 (pb.translation[b], r.translation[0], "ds_dtranslation")):
                assert bool(torch.isfinite(got).all()), f"{w}[{b}]"
                assert_close(got, want, tol(np.float32, "pose"), f"{w}[{b}]")


# ------------------------------------------------------------------ 5. the inputs are what they claim (no device)
def expectations():
    """key -> (expected, spans of the scopes by field) of every entry of RHO"""
    for name, case in JVP_CASES:
        yield ("jvp", case, name), jvp_expected(name, case)
    for name in ("W3", "W2_32"):
        for case in ("wide", "bg"):
            yield ("channels", case, name), channel_expected(name, case)
    for gname, P, case in CLOUD_CASES:
        yield ("clouds", case, gname, P), cloud_expected(gname, P, case)
    for name in ("W3", "W2_32"):
        yield ("sample", name), sample_expected(name)


def measure_rho(e):
    """rho of the module docstring from one family's expectation (all its planes)"""
    return worst_ratio(e.ref32, e.ref64, e.S)


@pytest.mark.parametrize("name", list(SPEC))
def test_no_tile_is_split(name):
    h = wide_input(name)
    for b in range(3):
        counts = tile_counts(h.grid, h.points, h.rot[b], h.trans[b])
        print(f"{name} pose {b}: {counts.size} tiles of {TILE[h.n_out]}, heaviest {counts.max()}")
        assert counts.max() <= CAP[h.n_out], (name, b, counts.max())
        assert counts.size > 1 and not cells(name, b)[0][-FAR:].any()
    assert cells(name, 0)[0][:-FAR].all() and not cells(name, 1)[0][:-FAR].all()  # (the other poses reject some)


def test_inputs_are_in_the_regime_they_claim():
    """The span of the magnitudes per scope: above 2^20 for `wide` / `slabs`, below 2^10 for `narrow` and `tiny`."""
    wide, narrow = (lambda x: np.all(np.asarray(x) > 2.0 ** 20)), (lambda x: np.all(np.asarray(x) < 2.0 ** 10))
    for name in ("W3", "W2_32", "W2_22"):
        sp = jvp_expected(name, "a").spans  # tangents wide, tiny, narrow
        assert wide(sp[0]) and narrow(sp[1]) and narrow(sp[2]), (name, sp)
    for name in ("W3", "W2_32"):
        assert wide(jvp_expected(name, "b").spans[0]), name  # slabs x N(0, 1)
        assert wide(jvp_expected(name, "c_wide").spans) and narrow(jvp_expected(name, "c_narrow").spans), name
        assert narrow(jvp_expected(name, "bg").spans), name
        sp = channel_expected(name, "wide").spans  # channels wide, tiny, narrow, slabs
        assert wide(sp[0]) and narrow(sp[1]) and narrow(sp[2]) and wide(sp[3]), (name, sp)
        assert narrow(channel_expected(name, "bg").spans), name
        sp = sample_expected(name).spans  # columns wide, tiny, narrow
        assert wide(sp[0]) and narrow(sp[1]) and narrow(sp[2]), (name, sp)
    for gname, P, case in CLOUD_CASES:
        sp = cloud_expected(gname, P, case).spans
        if case == "perpose":  # poses wide, tiny, narrow
            assert wide(sp[0]) and narrow(sp[1]) and narrow(sp[2]), (gname, P, sp)
        else:
            assert wide(sp) if case == "shared" else narrow(sp), (gname, P, case, sp)


def test_rho_table_is_reproducible_and_the_reference_meets_its_own_bound():
    """Every rho of the table is what `measure_rho` gives today (to the table's digits); ref32 is within 4 rho of
    ref64 on every cell with S > 0 and holds the background's bits where S = 0 -- which also pins S's cell choice
    to the oracle's fp32 cells."""
    keys = []
    for key, e in expectations():
        keys.append(key)
        rho = measure_rho(e)
        assert abs(rho - RHO[key]) <= 1e-3 * RHO[key], (key, rho, RHO[key])
        assert rho <= M_FACTOR * RHO[key]
        bg = getattr(e, "bg", None)
        if bg is None and key[1] != "bg":
            assert bits_equal(e.ref32[e.S == 0], 0.0), key
        elif bg is not None:
            want = np.broadcast_to(np.asarray(bg, np.float32), e.S.shape)
            assert np.array_equal(np.asarray(e.ref32, np.float32)[e.S == 0], want[e.S == 0]), key
    assert sorted(keys) == sorted(RHO)


if __name__ == "__main__":
    for key, e in expectations():
        print(f"    {' / '.join(map(str, key)):<32} {measure_rho(e):.3e}")
