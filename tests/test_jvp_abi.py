"""Host-side checks of the forward-mode derivative (include/dpr.h, FORWARD-MODE DERIVATIVE): prototypes and
exports, workspace sizes, the AUTO rule, argument errors -- and a numpy restatement of the definition, pinned
against the oracle's Jacobian (J . v from `oracle.raster_pullback`) and central differences of `oracle.raster`.
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpr_amd
from dpr_amd import _lib
from tests import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_raster_jvp_ex_f32", "dpr_raster_jvp_ex_f64", "dpr_workspace_bytes_jvp_ex_f32",
       "dpr_workspace_bytes_jvp_ex_f64", "dpr_resolve_algo_jvp"]
SIZE_MAX = ctypes.c_size_t(-1).value
C3 = (256, 256, 256)
PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
KINDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ the definition, restated in numpy
def jvp_reference(grid, points, rot, trans, ow, pw, tan, K, cell_dtype=np.float64, value_dtype=np.float64):
    """out_dot (grid..., K, B) in fp64 of the JVP definition in include/dpr.h.  rot (B, N_out, N_in),
    trans (B, N_out), ow (B,) / None, pw (P,) / None; tan: dict kind -> array with a leading K axis (points
    (K, P, N_in), rotation (K, B, N_out, N_in), translation (K, B, N_out), background / out_weight (K, B),
    point_weight (K, P)); missing kinds are zero.  Rejected points read none of their tangents.
    cell_dtype: the precision of the cell choice and the deltas (np.float32: the library's fp32 cells, bit for
    bit); everything after them is fp64 -- or value_dtype: np.float32 gives the restatement's own fp32 rounding
    (every deposit and every running cell sum in fp32, points in index order), the yardstick of an fp32 result."""
    ct = np.dtype(cell_dtype)
    vt = np.dtype(value_dtype)
    pts_c = np.asarray(points, ct)
    rot_c = np.asarray(rot, ct)
    trans_c = np.asarray(trans, ct)
    points = np.asarray(points, vt)
    rot = np.asarray(rot, vt)
    trans = np.asarray(trans, vt)
    P, n_in = points.shape
    B, n_out = rot.shape[0], rot.shape[1]
    ow = np.ones(B, vt) if ow is None else np.asarray(ow, vt)
    pw = np.ones(P, vt) if pw is None else np.asarray(pw, vt)
    z = lambda shape: np.zeros(shape, vt)
    t = lambda kind, shape: np.asarray(tan[kind], vt) if kind in tan else z(shape)
    pd = t("points", (K, P, n_in))
    rd = t("rotation", (K, B, n_out, n_in))
    td = t("translation", (K, B, n_out))
    bgd = t("background", (K, B))
    owd = t("out_weight", (K, B))
    pwd = t("point_weight", (K, P))
    out = np.zeros(tuple(grid) + (K, B), vt, order="F")
    n = np.asarray(grid, vt)
    for b in range(B):
        # cell and deltas in the library's (the reference's) operation order
        coord = np.empty((P, n_out), dtype=ct)
        for d in range(n_out):
            proj = rot_c[b, d, 0] * pts_c[:, 0]
            for j in range(1, n_in):
                proj = proj + rot_c[b, d, j] * pts_c[:, j]
            coord[:, d] = (proj - (ct.type(-1.0) - trans_c[b, d])) * (ct.type(grid[d]) / ct.type(2))
        c = coord - ct.type(0.5)
        ok = np.all((c > -1) & (c <= n.astype(ct)), axis=1)
        r = np.ceil(np.where(ok[:, None], c, ct.type(0.0)))
        ref0 = r.astype(np.int64) - 1
        dlo = (coord - (r - ct.type(0.5))).astype(vt)
        q = np.nonzero(ok)[0]
        for k in range(K):
            out[..., k, b] = bgd[k, b]
            if q.size == 0:
                continue
            cdot = (np.einsum("nj,pj->pn", rd[k, b], points[q]) + np.einsum("nj,pj->pn", rot[b], pd[k, q])
                    + td[k, b][None, :]) * (n / 2)[None, :]
            a = owd[k, b] * pw[q] + ow[b] * pwd[k, q]
            bn = (ow[b] * pw[q])[:, None] * cdot
            dl = dlo[q]
            plane = out[..., k, b]
            for s in range(1 << n_out):
                bits = np.array([(s >> d) & 1 for d in range(n_out)])
                fac = np.where(bits[None, :] == 1, dl, vt.type(1.0) - dl)
                dep = a * np.prod(fac, axis=1)
                for m in range(n_out):
                    others = np.prod(np.delete(fac, m, axis=1), axis=1) if n_out > 1 else np.ones(q.size, vt)
                    dep = dep + bn[:, m] * vt.type(1.0 if bits[m] else -1.0) * others
                idx = ref0[q] + bits[None, :]
                inb = np.all((idx >= 0) & (idx < np.asarray(grid)[None, :]), axis=1)
                np.add.at(plane, tuple(idx[inb].T), dep[inb])
            out[..., k, b] = plane
    return out


def cell_choice(grid, points, rot_b, trans_b, cell_dtype=np.float64):
    """(ok (P,), ref0 (P, N_out), coord (P, N_out)) of one pose in `jvp_reference`'s operation order (np.float32:
    the library's fp32 cells, bit for bit); rejected points have ref0 = -1."""
    ct = np.dtype(cell_dtype)
    pts, R, t = np.asarray(points, ct), np.asarray(rot_b, ct), np.asarray(trans_b, ct)
    n_out, n_in = R.shape
    coord = np.empty((len(pts), n_out), dtype=ct)
    for d in range(n_out):
        proj = R[d, 0] * pts[:, 0]
        for j in range(1, n_in):
            proj = proj + R[d, j] * pts[:, j]
        coord[:, d] = (proj - (ct.type(-1.0) - t[d])) * (ct.type(grid[d]) / ct.type(2))
    with np.errstate(invalid="ignore"):
        c = coord - ct.type(0.5)
        ok = np.all((c > -1) & (c <= np.asarray(grid, ct)), axis=1)
        ref0 = np.ceil(np.where(ok[:, None], c, ct.type(0.0))).astype(np.int64) - 1
    return ok, ref0, coord


def footprint_sum(grid, ok, ref0, mag):
    """S (grid...) in fp64: the sum of mag[p] over the accepted points p that touch the cell with any of their
    2^N corners ref0 + {0, 1}^N."""
    S = np.zeros(tuple(grid), np.float64)
    q = np.nonzero(ok)[0]
    n_out = ref0.shape[1]
    m = np.asarray(mag, np.float64)[q]
    for s in range(1 << n_out):
        idx = ref0[q] + np.array([(s >> d) & 1 for d in range(n_out)])[None, :]
        inb = np.all((idx >= 0) & (idx < np.asarray(grid)[None, :]), axis=1)
        np.add.at(S, tuple(idx[inb].T), m[inb])
    return S


def jvp_terms(grid, points, rot, trans, ow, pw, tan, K, b, cell_dtype=np.float64):
    """(ok (P,), ref0 (P, N_out), a (K, P), bn (K, P, N_out)) of pose b: the coefficients of `jvp_reference`'s
    deposits (include/dpr.h: deposit = a * prod + sum_n b_n * d prod / d delta_n) in fp64, zero on rejected
    points.  |a| + sum_n |b_n| is the bound the tiled JVP scales its fixed-point sums by."""
    points, rot, trans = (np.asarray(x, np.float64) for x in (points, rot, trans))
    P, n_in = points.shape
    B, n_out = rot.shape[0], rot.shape[1]
    ow = np.ones(B) if ow is None else np.asarray(ow, np.float64)
    pw = np.ones(P) if pw is None else np.asarray(pw, np.float64)
    t = lambda kind, shape: np.asarray(tan[kind], np.float64) if kind in tan else np.zeros(shape)
    pd, rd, td = t("points", (K, P, n_in)), t("rotation", (K, B, n_out, n_in)), t("translation", (K, B, n_out))
    owd, pwd = t("out_weight", (K, B)), t("point_weight", (K, P))
    ok, ref0, _ = cell_choice(grid, points, rot[b], trans[b], cell_dtype)
    a, bn = np.zeros((K, P)), np.zeros((K, P, n_out))
    q = np.nonzero(ok)[0]
    n = np.asarray(grid, np.float64)
    for k in range(K):
        cdot = (np.einsum("nj,pj->pn", rd[k, b], points[q]) + np.einsum("nj,pj->pn", rot[b], pd[k, q])
                + td[k, b][None, :]) * (n / 2)[None, :]
        a[k, q] = owd[k, b] * pw[q] + ow[b] * pwd[k, q]
        bn[k, q] = (ow[b] * pw[q])[:, None] * cdot
    return ok, ref0, a, bn


def random_tangents(rng, K, P, B, n_in, n_out, kinds=KINDS):
    shapes = dict(points=(K, P, n_in), rotation=(K, B, n_out, n_in), translation=(K, B, n_out),
                  background=(K, B), out_weight=(K, B), point_weight=(K, P))
    return {k: rng.normal(size=shapes[k]) for k in kinds}


# ------------------------------------------------------------------ exports, workspace, AUTO, errors
def test_header_declares_and_library_exports_the_jvp_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert L.dpr_version() >= 108
    for name in ("raster_jvp", "raster_jvp_", "resolve_algo_jvp", "workspace_bytes_jvp"):
        assert callable(getattr(dpr_amd, name)), name


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes_jvp(suf):
    f = getattr(dpr_amd.lib(), f"dpr_workspace_bytes_jvp_ex_{suf}")
    a, gp = _g(C3)
    P = 10_000_000
    for n_in, n_out in PAIRS:
        ag, gg = _g((16,) * n_out)
        for K in (1, 16):
            assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gg, 1000, 3, K) == 0, (n_in, n_out, K)
    n1 = f(_lib.ALGO_TILED, 0, 3, 3, gp, P, 1, 1)
    assert 0 < n1 < SIZE_MAX
    # independent of B and K
    assert f(_lib.ALGO_TILED, 0, 3, 3, gp, P, 8, 12) == n1
    for grid, n_in in (((512, 512), 3), ((512, 512), 2)):
        ag, gg = _g(grid)
        assert 0 < f(_lib.ALGO_TILED, 0, n_in, 2, gg, P, 8, 12) < SIZE_MAX
    # refused: K out of range, bad dims, tiled on a direct-only pair or a multi-slab grid, chunked, KEEP / REUSE
    for K in (0, 17, -1):
        assert f(_lib.ALGO_ATOMIC, 0, 3, 3, gp, P, 1, K) == SIZE_MAX
    assert f(_lib.ALGO_ATOMIC, 0, 5, 3, gp, P, 1, 1) == SIZE_MAX
    assert f(_lib.ALGO_ATOMIC, 0, 3, 0, gp, P, 1, 1) == SIZE_MAX
    a2, gp2 = _g((64, 64, 64))
    assert f(_lib.ALGO_TILED, 0, 2, 3, gp2, P, 1, 1) == SIZE_MAX
    a3, gp3 = _g((1024, 1024, 1024))
    assert f(_lib.ALGO_TILED, 0, 3, 3, gp3, P, 1, 1) == SIZE_MAX
    assert f(_lib.ALGO_CHUNKED, 0, 3, 3, gp, P, 1, 1) == SIZE_MAX
    assert f(_lib.ALGO_AUTO, _lib.FLAG_KEEP_BINNING, 3, 3, gp, P, 1, 1) == SIZE_MAX
    assert f(_lib.ALGO_AUTO, _lib.FLAG_REUSE_BINNING, 3, 3, gp, P, 1, 1) == SIZE_MAX
    # the Python mirror
    import torch

    dt = {"f32": torch.float32, "f64": torch.float64}[suf]
    assert dpr_amd.workspace_bytes_jvp(C3, P, 1, 3, 1, dt, "tiled") == n1
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes_jvp(C3, P, 1, 3, 17, dt)


def test_resolve_algo_jvp():
    # pinned shapes, then the rule itself over a table
    assert dpr_amd.resolve_algo_jvp(C3, 10_000_000, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo_jvp(C3, 10_000_000, 8, 3, 12) == "tiled"
    assert dpr_amd.resolve_algo_jvp((64,) * 3, 10_000_000, 1, 2) == "atomic"  # (2, 3): direct kernels only
    assert dpr_amd.resolve_algo_jvp((16,) * 4, 100_000, 1, 4) == "atomic"
    assert dpr_amd.resolve_algo_jvp((1024,) * 3, 10_000_000, 1, 3) == "atomic"  # several tile slabs
    table = [((256,) * 3, 10_000_000, 1, 3), ((128,) * 3, 1_000_000, 1, 3), ((512, 512), 10_000_000, 8, 3),
             ((512, 512), 1_000_000, 8, 2), ((64, 64), 1000, 1, 2), ((32,) * 3, 100, 3, 3), ((16, 16), 10, 1, 3)]
    for grid, P, B, n_in in table:
        single = dpr_amd.resolve_algo("raster", grid, P, 1, n_in)
        want = "tiled" if single == "tiled" else "atomic"
        for K in (1, 5, 16):
            assert dpr_amd.resolve_algo_jvp(grid, P, B, n_in, K) == want, (grid, P, B, n_in, K)
    a, gp = _g(C3)
    L = dpr_amd.lib()
    assert L.dpr_resolve_algo_jvp(3, 3, gp, 1000, 1, 0) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_jvp(3, 3, gp, 1000, 1, 17) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_jvp(5, 3, gp, 1000, 1, 1) == _lib.ERR_UNSUPPORTED_DIMS


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_bad_arguments_are_refused_before_any_launch(suf):
    """Every refusal happens on the host: fake device pointers are never dereferenced (no GPU here)."""
    fn = getattr(dpr_amd.lib(), f"dpr_raster_jvp_ex_{suf}")
    fake = ctypes.c_void_p(1 << 20)  # aligned, never touched
    a, gp = _g((16, 16, 16))

    def call(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, grid=gp, P=100, B=2, K=1, out=fake, pts=fake,
             rot=fake, trans=fake, ws=None, ws_bytes=0):
        return fn(None, algo, flags, n_in, n_out, grid, P, B, K, out, pts, rot, trans, None, None, fake, fake,
                  fake, fake, fake, fake, ws, ws_bytes)

    assert call(n_in=5) == _lib.ERR_UNSUPPORTED_DIMS
    assert call(n_out=0) == _lib.ERR_UNSUPPORTED_DIMS
    assert call(grid=None) == _lib.ERR_INVALID_ARG
    assert call(K=0) == _lib.ERR_INVALID_ARG
    assert call(K=17) == _lib.ERR_INVALID_ARG
    assert call(out=None) == _lib.ERR_INVALID_ARG
    assert call(pts=None) == _lib.ERR_INVALID_ARG
    assert call(rot=None) == _lib.ERR_INVALID_ARG
    assert call(trans=None) == _lib.ERR_INVALID_ARG
    assert call(algo=_lib.ALGO_CHUNKED) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(algo=_lib.ALGO_TILED, n_in=2) == _lib.ERR_UNSUPPORTED_ALGO
    a4, gp4 = _g((1024, 1024, 1024))
    assert call(algo=_lib.ALGO_TILED, grid=gp4) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(flags=_lib.FLAG_KEEP_BINNING) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(flags=_lib.FLAG_REUSE_BINNING) == _lib.ERR_UNSUPPORTED_ALGO
    assert call(algo=_lib.ALGO_TILED) == _lib.ERR_WORKSPACE
    assert call(algo=_lib.ALGO_TILED, ws=ctypes.c_void_p(1 << 20), ws_bytes=256) == _lib.ERR_WORKSPACE
    assert "workspace" in _lib.last_error()
    # nothing to do is not an error (and launches nothing)
    assert call(B=0) == _lib.OK


def test_python_refuses_cpu_tensors():
    import torch

    pts = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster_jvp((8, 8, 8), pts, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                           points_dot=pts)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.raster_jvp((8, 8, 8), pts, torch.eye(3), torch.zeros(3), tangents=17)


# ------------------------------------------------------------------ the restatement against the oracle
def _problem(n_in, n_out, B, P, seed, faces=False):
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B, grid_n=8, seed=seed)
    rng = np.random.default_rng(seed + 1)
    grid = {1: (8,), 2: (8, 8), 3: (6, 6, 6), 4: (4, 4, 4, 4)}[n_out]
    points, rot, trans = d.points.copy(), d.rotations.copy(), d.translations.copy()
    ow = rng.uniform(0.5, 2.0, size=B)
    pw = rng.uniform(0.5, 2.0, size=P)
    if faces:
        # an identity-like pose (first N_out rows of I) without translation on a grid of 8 per axis: points at
        # half-integer coordinates sit exactly on cell faces (dlo = 1, ref0 one below)
        grid = (8,) * n_out
        rot[:] = np.eye(n_out, n_in)[None]
        trans[:] = 0.0
        half = rng.integers(0, 8, size=(P, n_in)) + 0.5  # coordinate in [0.5, 7.5]
        points = 2.0 * half / 8.0 - 1.0
    return grid, points, rot, trans, ow, pw


def _jacobian(grid, points, rot, trans, ow, pw):
    """Rows of J (one per output cell of (grid..., B)) from the oracle's pullback with unit ds_dout, columns
    in the order points, rotation, translation, background, out_weight, point_weight."""
    from oracle import oracle

    B = rot.shape[0]
    G = int(np.prod(grid))
    rows = []
    for i in range(G * B):
        e = np.zeros(G * B)
        e[i] = 1.0
        pb = oracle.raster_pullback(e.reshape(tuple(grid) + (B,), order="F"), points, rot, trans, ow, pw)
        rows.append(np.concatenate([pb.points.ravel(), pb.rotation.ravel(), pb.translation.ravel(),
                                    pb.background.ravel(), pb.out_weight.ravel(), pb.point_weight.ravel()]))
    return np.asarray(rows)


def _tangent_vector(tan, k, shapes):
    parts = []
    for kind in KINDS:
        parts.append(tan[kind][k].ravel() if kind in tan else np.zeros(int(np.prod(shapes[kind]))))
    return np.concatenate(parts)


def _to_grid_b(out_dot, k):
    """plane k of out_dot (grid..., K, B) as the flat column-major (grid..., B) vector J rows index."""
    return np.asarray(out_dot[..., k, :]).ravel(order="F")


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_restatement_equals_the_oracle_jacobian(n_in, n_out, oracle):
    rng = np.random.default_rng(100 * n_in + n_out)
    B, P, K = 2, 12, 3
    for faces in (False, True):
        grid, points, rot, trans, ow, pw = _problem(n_in, n_out, B, P, seed=n_in * 7 + n_out, faces=faces)
        # two rejected points (far outside every grid) whose tangents are NaN
        points = np.concatenate([points, np.full((2, n_in), 9.0)])
        pw = np.concatenate([pw, [1.0, 1.0]])
        Pt = P + 2
        J = _jacobian(grid, points, rot, trans, ow, pw)
        shapes = dict(points=(Pt, n_in), rotation=(B, n_out, n_in), translation=(B, n_out), background=(B,),
                      out_weight=(B,), point_weight=(Pt,))
        for kinds in [(k,) for k in KINDS] + [KINDS]:
            tan = random_tangents(rng, K, Pt, B, n_in, n_out, kinds)
            clean = {k: v.copy() for k, v in tan.items()}
            for kind in ("points", "point_weight"):
                if kind in tan:
                    tan[kind][:, P:] = np.nan  # the rejected points: never read
                    clean[kind][:, P:] = 0.0
            got = jvp_reference(grid, points, rot, trans, ow, pw, tan, K)
            assert np.all(np.isfinite(got)), (faces, kinds)
            for k in range(K):
                want = J @ _tangent_vector(clean, k, shapes)
                a = _to_grid_b(got, k)
                err = np.linalg.norm(a - want)
                assert err <= 1e-12 * max(np.linalg.norm(want), 1e-300) + 1e-300, (faces, kinds, k, err)


@pytest.mark.parametrize("n_in,n_out", [(3, 3), (3, 2), (2, 2), (1, 1), (4, 4), (2, 3)])
def test_restatement_matches_central_differences_of_the_oracle(n_in, n_out, oracle):
    rng = np.random.default_rng(5)
    B, P, K = 2, 40, 1
    grid, points, rot, trans, ow, pw = _problem(n_in, n_out, B, P, seed=3)
    bg = rng.normal(size=B)
    tan = random_tangents(rng, K, P, B, n_in, n_out)
    got = jvp_reference(grid, points, rot, trans, ow, pw, tan, K)[..., 0, :]
    h = 1e-7

    def f(sign):
        return oracle.raster(grid, points + sign * h * tan["points"][0], rot + sign * h * tan["rotation"][0],
                             trans + sign * h * tan["translation"][0], bg + sign * h * tan["background"][0],
                             ow + sign * h * tan["out_weight"][0], pw + sign * h * tan["point_weight"][0])

    fd = (f(1.0) - f(-1.0)) / (2 * h)
    assert np.linalg.norm(fd - got) <= 1e-6 * np.linalg.norm(got)
