"""Host-side checks of the rigid-body C ABI (include/dpr.h, RIGID BODIES): prototypes and exports, the workspace
query, every refusal, the Python shape checks, and the reference composition of tests/bodies_reference.py against the
oracle it is made of.  No GPU needed: every refused call returns before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib
from oracle import oracle
from tests import bodies_reference as ref
from tests import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_raster_bodies_ex_f32", "dpr_raster_bodies_ex_f64", "dpr_raster_pullback_bodies_ex_f32",
       "dpr_raster_pullback_bodies_ex_f64", "dpr_workspace_bytes_bodies_ex_f32", "dpr_workspace_bytes_bodies_ex_f64",
       "dpr_resolve_algo_bodies"]
NAMES = ["raster_bodies", "raster_bodies_", "raster_pullback_bodies_", "raster_bodies_ad", "resolve_algo_bodies"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
OPS = (_lib.OP_RASTER, _lib.OP_PULLBACK)


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_body_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    assert "RIGID BODIES" in open(os.path.join(ROOT, "include", "dpr.h")).read()
    L = dpr_amd.lib()
    assert len(NEW) == 7 and len(NAMES) == 5
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in NAMES:
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    assert L.dpr_version() == 110
    # no workspace, so no public query: tests/test_workspace_contract_table.py holds that list to its own table
    assert not any("bodies" in n for n in dir(dpr_amd) if n.startswith("workspace_bytes"))


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_query_is_zero_for_accepted_calls_and_refuses_the_rest(suf):
    f = getattr(dpr_amd.lib(), f"dpr_workspace_bytes_bodies_ex_{suf}")
    for n_in, n_out in PAIRS:
        a, gp = _g((16, 12, 10)[:n_out])
        for op in OPS:
            for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC):
                for P, B, K in ((1000, 3, 4), (0, 3, 1), (1000, 0, 2), (0, 0, 1), (10**9, 64, 1 << 20)):
                    assert f(op, algo, 0, n_in, n_out, gp, P, B, K) == 0, (op, algo, P, B, K)
                for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS):
                    assert f(op, algo, fl, n_in, n_out, gp, 1000, 3, 4) == 0
            for algo in (_lib.ALGO_TILED, _lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING, _lib.flag_max_pose_group(2)):
                assert f(op, _lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            for K in (0, -1):
                assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, K) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1, 1 << 31) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1 << 16, 1 << 15) == SIZE_MAX  # B * K = 2^31
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, (1 << 16) - 1, 1 << 15) == 0
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, -1, 3, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 10, -1, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, None, 10, 1, 4) == SIZE_MAX
        assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        assert f(7, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 2) == SIZE_MAX, (n_in, n_out)


def test_resolve_algo_bodies_answers_atomic():
    L = dpr_amd.lib()
    for n_in, n_out in PAIRS:
        grid = (128, 96, 64)[:n_out]
        a, gp = _g(grid)
        for op, opc in (("raster", _lib.OP_RASTER), ("pullback", _lib.OP_PULLBACK)):
            for P, B, K in ((0, 1, 1), (1000, 1, 1), (10**7, 64, 16), (10**5, 1000, 5000)):
                assert L.dpr_resolve_algo_bodies(opc, n_in, n_out, gp, P, B, K) == _lib.ALGO_ATOMIC
                assert dpr_amd.resolve_algo_bodies(op, grid, P, B, K, n_in) == "atomic"
    a, gp = _g((64, 64))
    assert L.dpr_resolve_algo_bodies(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_ALGO
    assert L.dpr_resolve_algo_bodies(9, 3, 2, gp, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_bodies(_lib.OP_RASTER, 0, 2, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert L.dpr_resolve_algo_bodies(_lib.OP_RASTER, 2, 3, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert L.dpr_resolve_algo_bodies(_lib.OP_RASTER, 3, 2, gp, 100, 2, 0) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_bodies(_lib.OP_RASTER, 3, 2, None, 100, 2, 2) == _lib.ERR_INVALID_ARG
    with pytest.raises(KeyError):
        dpr_amd.resolve_algo_bodies("residual_pullback", (64, 64), 100, 2, 2, 3)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_bodies("raster", (64, 64), 100, 2, 0, 3)


def test_body_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy aligned device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_bodies_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_bodies_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, out=d, pts=d, body=d, rot=d, trans=d,
              grid=gp, ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, K, out, pts, body, rot, trans, None, None, None,
                       ws, wsb)

        def b(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, g=d, pts=d, body=d, rot=d, trans=d,
              outs=(d, d, d, d, d, d), ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, gp, P, B, K, g, pts, body, rot, trans, None, None, *outs, ws,
                       wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        for call in (f, b):
            # a pair other than the three, or K < 1
            refused(call(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
            refused(call(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
            for n_in, n_out in ALL_PAIRS:
                if (n_in, n_out) not in PAIRS:
                    refused(call(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
            refused(call(K=0), _lib.ERR_INVALID_ARG, "at least one body")
            refused(call(K=-3), _lib.ERR_INVALID_ARG, "at least one body")
            # B * K beyond the range the kernels index with
            refused(call(B=1 << 16, K=1 << 15), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
            refused(call(B=1, K=1 << 31), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
            refused(call(B=-1), _lib.ERR_INVALID_ARG, "negative")
            refused(call(P=-1), _lib.ERR_INVALID_ARG, "negative")
            # NULL points, body, rotation or translation while P * B > 0
            refused(call(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
            refused(call(body=None), _lib.ERR_INVALID_ARG, "body is NULL")
            refused(call(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
            refused(call(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
            # misaligned pointers
            refused(call(pts=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(rot=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(body=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(ws=odd, wsb=1024), _lib.ERR_WORKSPACE, "256-byte aligned")
            # any algorithm other than AUTO or ATOMIC: the message names the one there is
            for algo in (_lib.ALGO_TILED, _lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                refused(call(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC")
            # the binning and pose-group flags
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                refused(call(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            refused(call(flags=_lib.flag_max_pose_group(4)), _lib.ERR_UNSUPPORTED_ALGO, "pose groups")
            # refusals come before the empty-batch return
            refused(call(B=0, P=0, algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC")
            refused(call(B=0, P=0, K=0), _lib.ERR_INVALID_ARG, "at least one body")
            # P = 0 and B = 0 together: valid, empty, nothing to launch
            assert call(B=0, P=0) == _lib.OK
        refused(f(out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        refused(f(out=odd), _lib.ERR_INVALID_ARG, "aligned")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        refused(b(g=None), _lib.ERR_INVALID_ARG, "ds_dout is NULL")
        refused(b(outs=(d, None, d, d, d, d)), _lib.ERR_INVALID_ARG, "per-pose output")
        refused(b(outs=(None, d, d, d, d, d)), _lib.ERR_INVALID_ARG, "ds_dpoints")
        refused(b(outs=(d, d, d, d, d, None)), _lib.ERR_INVALID_ARG, "ds_dpoint_weight")
        refused(b(outs=(d, d, odd, d, d, d)), _lib.ERR_INVALID_ARG, "aligned")
        # a NULL forward input with no (point, image) pair to read it is no error
        assert f(B=0, pts=None, body=None, rot=None, trans=None, out=None) == _lib.OK


def test_python_wrappers_raise_without_a_device():
    pts, body = torch.zeros(10, 3), torch.zeros(10, dtype=torch.int64)
    R, t = torch.zeros(4, 2, 2, 3), torch.zeros(4, 2, 2)
    bad = [
        dict(points=torch.zeros(4, 10, 3)),                          # not (P, N_in)
        dict(points=torch.zeros(10, 2)),                             # N_in differs from rotation's columns
        dict(body=torch.zeros(9, dtype=torch.int64)),                # P differs
        dict(body=torch.zeros(10, 1, dtype=torch.int32)),            # not (P,)
        dict(rotation=torch.zeros(2, 3)),                            # no K axis
        dict(rotation=torch.zeros(4, 0, 2, 3), translation=torch.zeros(4, 0, 2)),   # K = 0
        dict(translation=torch.zeros(4, 2, 3)),                      # N_out differs
        dict(translation=torch.zeros(3, 2, 2)),                      # B differs
        dict(translation=torch.zeros(4, 3, 2)),                      # K differs
        dict(translation=torch.zeros(4, 2)),                         # no K axis
        dict(rotation=torch.zeros(4, 2, 3, 2), points=torch.zeros(10, 2), translation=torch.zeros(4, 2, 3)),  # (2, 3)
        dict(rotation=torch.zeros(4, 2, 1, 3), translation=torch.zeros(4, 2, 1)),                              # (3, 1)
        dict(point_weight=torch.ones(9)),
    ]
    for kw in bad:
        a = dict(points=pts, body=body, rotation=R, translation=t, point_weight=None)
        a.update(kw)
        args = (a["points"], a["body"], a["rotation"], a["translation"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_bodies((16, 16), *args, point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_pullback_bodies_(torch.zeros(16, 16, 4), *args, point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_bodies_ad((16, 16), *args, point_weight=a["point_weight"])
    with pytest.raises(TypeError):
        dpr_amd.raster_bodies((16, 16), pts, body.float(), R, t)
    # consistent shapes on the CPU: the error of `raster`
    for call in (lambda: dpr_amd.raster_bodies((16, 16), pts, body, R, t),
                 lambda: dpr_amd.raster_bodies((16, 16), pts, body, R[0], t[0]),
                 lambda: dpr_amd.raster_bodies_(torch.zeros(16, 16, 4), pts, body, R, t),
                 lambda: dpr_amd.raster_pullback_bodies_(torch.zeros(16, 16, 4), pts, body, R, t),
                 lambda: dpr_amd.raster_bodies_ad((16, 16), pts, body, R, t)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ------------------------------------------------------------------ the reference composition itself
def _problem(n_in, n_out, B, K, P, grid, seed):
    rng = np.random.default_rng(seed)
    d = D.make(n_points=P, n_in=n_in, n_out=n_out, batch=B * K, grid_n=grid, seed=seed)
    return dict(grid=tuple(grid), points=d.points, body=rng.integers(0, K, size=P),
                rot=d.rotations.reshape(B, K, n_out, n_in), trans=d.translations.reshape(B, K, n_out),
                bg=np.arange(1, B + 1, dtype=np.float64), ow=rng.uniform(1, 10, size=B),
                pw=rng.uniform(0.5, 1.5, size=P), ds=rng.normal(size=tuple(grid) + (B,)))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_for_one_body_the_reference_is_the_oracle(n_in, n_out, npdt):
    c = _problem(n_in, n_out, B=3, K=1, P=300, grid=(9, 7, 5)[:n_out], seed=n_in + n_out)
    body = np.zeros(300, dtype=np.int64)
    want = oracle.raster(c["grid"], c["points"], c["rot"][:, 0], c["trans"][:, 0], None, c["ow"], c["pw"], dtype=npdt)
    got = ref.raster(c["grid"], c["points"], body, c["rot"], c["trans"], None, c["ow"], c["pw"], dtype=npdt)
    assert np.array_equal(got, want)
    # the background is added behind the sum, the oracle starts from it: one rounding apart
    want = oracle.raster(c["grid"], c["points"], c["rot"][:, 0], c["trans"][:, 0], c["bg"], c["ow"], c["pw"],
                         dtype=npdt)
    got = ref.raster(c["grid"], c["points"], body, c["rot"], c["trans"], c["bg"], c["ow"], c["pw"], dtype=npdt)
    assert got.dtype == npdt
    assert np.abs(got - want).max() <= 8 * np.finfo(npdt).eps * np.abs(want).max()
    r = oracle.raster_pullback(c["ds"], c["points"], c["rot"][:, 0], c["trans"][:, 0], c["ow"], c["pw"], dtype=npdt)
    g = ref.raster_pullback(c["ds"], c["points"], body, c["rot"], c["trans"], c["ow"], c["pw"], dtype=npdt)
    assert g.rotation.shape == (3, 1, n_out, n_in) and g.translation.shape == (3, 1, n_out)
    for name in ("points", "background", "out_weight", "point_weight"):
        assert np.array_equal(getattr(g, name), getattr(r, name)), name
    assert np.array_equal(g.rotation[:, 0], r.rotation) and np.array_equal(g.translation[:, 0], r.translation)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_the_reference_does_not_change_when_points_and_body_are_permuted_together(n_in, n_out):
    c = _problem(n_in, n_out, B=2, K=4, P=400, grid=(9, 7, 5)[:n_out], seed=20 + n_in + n_out)
    c["body"][:7] = (-1, 4, 2**31 - 1, -5, 4, 9, -1)  # outside [0, K): in no subset
    perm = np.random.default_rng(1).permutation(400)
    a = ref.raster(c["grid"], c["points"], c["body"], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    b = ref.raster(c["grid"], c["points"][perm], c["body"][perm], c["rot"], c["trans"], c["bg"], c["ow"], c["pw"][perm])
    # (within a subset the points keep their relative order only up to the permutation: rounding level)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    ga = ref.raster_pullback(c["ds"], c["points"], c["body"], c["rot"], c["trans"], c["ow"], c["pw"])
    gb = ref.raster_pullback(c["ds"], c["points"][perm], c["body"][perm], c["rot"], c["trans"], c["ow"], c["pw"][perm])
    assert np.array_equal(ga.points[perm], gb.points) and np.array_equal(ga.point_weight[perm], gb.point_weight)
    assert np.array_equal(ga.background, gb.background)
    for name in ("rotation", "translation", "out_weight"):
        x, y = getattr(ga, name), getattr(gb, name)
        assert np.abs(x - y).max() <= 1e-12 * np.abs(x).max(), name
    assert (ga.points[:7] == 0).all() and (ga.point_weight[:7] == 0).all()
    # and the sum over the bodies is what one body per point set gives: K subsets against the whole cloud under one pose
    same = np.broadcast_to(c["rot"][:, :1], c["rot"].shape), np.broadcast_to(c["trans"][:, :1], c["trans"].shape)
    keep = (c["body"] >= 0) & (c["body"] < 4)
    whole = oracle.raster(c["grid"], c["points"][keep], c["rot"][:, 0], c["trans"][:, 0], c["bg"], c["ow"], c["pw"][keep])
    parts = ref.raster(c["grid"], c["points"], c["body"], *same, c["bg"], c["ow"], c["pw"])
    assert np.abs(parts - whole).max() <= 1e-13 * np.abs(whole).max()


def test_the_reference_of_a_cloud_without_accepted_points():
    c = _problem(3, 2, B=2, K=3, P=5, grid=(6, 5), seed=3)
    body = np.full(5, 7)
    out = ref.raster(c["grid"], c["points"], body, c["rot"], c["trans"], c["bg"], c["ow"], c["pw"])
    assert np.array_equal(out, np.broadcast_to(c["bg"], out.shape))
    g = ref.raster_pullback(c["ds"], c["points"], body, c["rot"], c["trans"], c["ow"], c["pw"])
    assert not g.points.any() and not g.rotation.any() and not g.translation.any() and not g.out_weight.any()
    assert np.allclose(g.background, c["ds"].sum(axis=(0, 1)), rtol=1e-13)
