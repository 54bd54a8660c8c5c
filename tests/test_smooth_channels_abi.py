"""Host-side checks of the C ABI of the smooth splat with channels (include/dpr.h, SMOOTH SPLAT, MULTI-CHANNEL):
prototypes and exports, workspace sizes, the AUTO rule against tests/golden/smooth_channels_auto.json, every refusal,
and the Python shape checks.  No GPU needed: every refused call returns before anything is launched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_raster_smooth_channels_ex_f32", "dpr_raster_smooth_channels_ex_f64",
       "dpr_raster_pullback_smooth_channels_ex_f32", "dpr_raster_pullback_smooth_channels_ex_f64",
       "dpr_workspace_bytes_smooth_channels_ex_f32", "dpr_workspace_bytes_smooth_channels_ex_f64",
       "dpr_resolve_algo_smooth_channels"]
PY = ["raster_smooth_channels", "raster_smooth_channels_", "raster_pullback_smooth_channels_",
      "raster_smooth_channels_ad", "resolve_algo_smooth_channels", "workspace_bytes_smooth_channels"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in PY:
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    assert "SMOOTH SPLAT, MULTI-CHANNEL" in open(os.path.join(ROOT, "include", "dpr.h")).read()
    assert L.dpr_version() == 110


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes_smooth_channels(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_smooth_channels_ex_{suf}")
    single = getattr(L, f"dpr_workspace_bytes_smooth_ex_{suf}")
    for n_in, n_out in PAIRS:
        a, gp = _g((37, 19, 21) if n_out == 3 else (150, 37))
        for C in (1, 3, 5, 16):
            # ATOMIC: no workspace, either op, whatever the accepted flags
            for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
                assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, C) == 0
                for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4)):
                    assert f(op, _lib.ALGO_ATOMIC, fl, n_in, n_out, gp, 1000, 3, C) == 0
                assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 0, 3, C) == 0
            # TILED forward: the smooth forward's workspace of the same (grid, P), whatever B and C
            for P in (1, 1000, 20_000, 1_000_000):
                want = single(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, 1)
                assert want not in (0, SIZE_MAX)
                for B in (1, 2, 16, 1000):
                    assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, B, C) == want
            assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 0, 4, C) == 0
            # the refused combinations
            assert f(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
            for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
                for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                    assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
                for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                    assert f(op, _lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
            assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
            assert f(7, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, -1, 3, C) == SIZE_MAX
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, -1, C) == SIZE_MAX
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, None, 10, 1, C) == SIZE_MAX
            assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 1, 1, C) == SIZE_MAX
            assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 2, 1, C) != SIZE_MAX
        for C in (0, 17, -1):
            for algo in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED, _lib.ALGO_AUTO):
                assert f(_lib.OP_RASTER, algo, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 3) == SIZE_MAX, (n_in, n_out)
    # the Python mirror
    assert dpr_amd.workspace_bytes_smooth_channels("pullback", (16, 16), 10, 2, 3, 4, algo="atomic") == 0
    assert dpr_amd.workspace_bytes_smooth_channels("raster", (16, 16), 10, 2, 3, 4, algo="tiled") == \
        dpr_amd.workspace_bytes_smooth("raster", (16, 16), 10, 1, 3, algo="tiled")
    for op, algo in (("pullback", "tiled"), ("raster", "chunked"), ("raster", "ordered")):
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.workspace_bytes_smooth_channels(op, (16, 16, 16), 10, 2, 3, 4, algo=algo)
    with pytest.raises(KeyError):
        dpr_amd.workspace_bytes_smooth_channels("residual_pullback", (16, 16), 10, 2, 3, 4)


def test_resolve_algo_smooth_channels_matches_the_recorded_table():
    """AUTO on the probe shapes (tests/golden/smooth_channels_auto.json: the choices, and the times
    profiles/smooth_channels_probe.txt recorded for both forward paths): one of the two algorithms, DPR_ALGO_TILED only
    where its workspace query succeeds, within 1.15x of the faster path on every recorded row (the margin
    tests/test_smooth_abi.py gives the smooth forward), the pullback always DPR_ALGO_ATOMIC."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_channels_auto.json")))
    L = dpr_amd.lib()
    timed = 0
    for row in table["shapes"]:
        a, gp = _g(row["grid"])
        n_out = len(row["grid"])
        for op, want in row["auto"].items():
            opc = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}[op]
            got = L.dpr_resolve_algo_smooth_channels(opc, row["n_in"], n_out, gp, row["P"], row["B"], row["C"])
            assert got == _lib.ALGOS[want], (row, op)
            assert dpr_amd.resolve_algo_smooth_channels(op, row["grid"], row["P"], row["B"], row["n_in"],
                                                        row["C"]) == want
            if "ms" in row and op in row["ms"]:
                t = row["ms"][op]
                assert set(t) == {"atomic", "tiled"}
                assert t[want] <= 1.15 * min(t.values()), (row["name"], op, t)
                timed += 1
        assert row["auto"]["pullback"] == "atomic"
    assert timed >= 18  # six shapes x three channel counts
    # never CHUNKED or ORDERED, TILED only where it can run, the pullback always ATOMIC, whatever the shape
    for n_in, n_out in PAIRS:
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 10**4, 10**5, 10**6, 10**7, 10**9, (1 << 32) - 1):
                for B in (1, 16, 1000):
                    for C in (1, 4, 16):
                        fw = L.dpr_resolve_algo_smooth_channels(_lib.OP_RASTER, n_in, n_out, gp, P, B, C)
                        assert fw in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED), (grid, P, B, C, fw)
                        if fw == _lib.ALGO_TILED:
                            q = L.dpr_workspace_bytes_smooth_channels_ex_f32(_lib.OP_RASTER, fw, 0, n_in, n_out, gp,
                                                                             P, B, C)
                            assert q != SIZE_MAX
                        assert L.dpr_resolve_algo_smooth_channels(_lib.OP_PULLBACK, n_in, n_out, gp, P, B,
                                                                  C) == _lib.ALGO_ATOMIC
    a, gp = _g((64, 64))
    r = L.dpr_resolve_algo_smooth_channels
    assert r(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2, 4) == _lib.ERR_UNSUPPORTED_ALGO
    assert r(9, 3, 2, gp, 100, 2, 4) == _lib.ERR_INVALID_ARG
    assert r(_lib.OP_RASTER, 0, 2, gp, 100, 2, 4) == _lib.ERR_UNSUPPORTED_DIMS
    assert r(_lib.OP_RASTER, 2, 3, gp, 100, 2, 4) == _lib.ERR_UNSUPPORTED_DIMS
    assert r(_lib.OP_RASTER, 3, 2, None, 100, 2, 4) == _lib.ERR_INVALID_ARG
    assert r(_lib.OP_RASTER, 3, 2, gp, 100, 2, 0) == _lib.ERR_INVALID_ARG
    assert r(_lib.OP_RASTER, 3, 2, gp, 100, 2, 17) == _lib.ERR_INVALID_ARG


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_smooth_channels_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_smooth_channels_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, C=3, out=d, pts=d, rot=d, trans=d, pw=d,
              grid=gp, ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, C, out, pts, rot, trans, None, None, pw, ws, wsb)

        def b(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, C=3, g=d, pts=d, rot=d, trans=d, pw=d,
              outs=(d, d, d, d, d, d), ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, gp, P, B, C, g, pts, rot, trans, None, pw, *outs, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        refused(f(out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        refused(f(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(f(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(pw=None), _lib.ERR_INVALID_ARG, "point_weight is NULL")
        refused(b(pw=None), _lib.ERR_INVALID_ARG, "point_weight is NULL")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        refused(f(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(P=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(out=odd), _lib.ERR_INVALID_ARG, "aligned")
        refused(f(pw=odd), _lib.ERR_INVALID_ARG, "aligned")
        refused(f(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        for C in (0, 17, -3):
            refused(f(C=C), _lib.ERR_INVALID_ARG, "out of range [1, 16]")
            refused(b(C=C), _lib.ERR_INVALID_ARG, "out of range [1, 16]")
        for n_in, n_out in ALL_PAIRS:
            if (n_in, n_out) not in PAIRS:
                refused(f(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
                refused(b(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            refused(f(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            refused(b(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            refused(f(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
            refused(b(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(b(algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "pullback runs on DPR_ALGO_ATOMIC only")
        # the tiled forward: no workspace, one too small, one misaligned
        need = getattr(L, f"dpr_workspace_bytes_smooth_channels_ex_{suf}")(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp,
                                                                           10, 2, 3)
        refused(f(algo=_lib.ALGO_TILED), _lib.ERR_WORKSPACE, "workspace")
        refused(f(algo=_lib.ALGO_TILED, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
        refused(f(algo=_lib.ALGO_TILED, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        refused(f(algo=_lib.ALGO_TILED, P=(1 << 32) - 1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")
        refused(b(g=None), _lib.ERR_INVALID_ARG, "ds_dout is NULL")
        refused(b(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(b(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(b(outs=(d, None, d, d, d, d)), _lib.ERR_INVALID_ARG, "per-pose output")
        refused(b(outs=(None, d, d, d, d, d)), _lib.ERR_INVALID_ARG, "ds_dpoints")
        refused(b(outs=(d, d, d, d, d, None)), _lib.ERR_INVALID_ARG, "ds_dpoint_weight")
        refused(b(outs=(d, d, odd, d, d, d)), _lib.ERR_INVALID_ARG, "aligned")
        refused(b(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        # the residual pullback is no op of this family (the queries take the op; the entry points are per op)
        wsq = getattr(L, f"dpr_workspace_bytes_smooth_channels_ex_{suf}")
        assert wsq(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 2, 3) == SIZE_MAX
        assert "no residual pullback" in _lib.last_error()
        # B = 0: nothing to do, after the checks
        assert f(B=0) == _lib.OK and b(B=0) == _lib.OK
        assert b(B=0, flags=_lib.FLAG_NO_POINT_WEIGHT_GRAD, outs=(d, d, d, d, d, None)) == _lib.OK
        refused(f(B=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(f(B=0, C=17), _lib.ERR_INVALID_ARG, "out of range")


def test_python_wrappers_raise_without_a_device():
    pts = torch.zeros(10, 3)
    R, t = torch.zeros(4, 2, 3), torch.zeros(4, 2)
    pw = torch.zeros(10, 3)
    bad = [
        dict(point_weight=torch.zeros(10)),                  # not (P, C)
        dict(point_weight=torch.zeros(9, 3)),                # P differs
        dict(point_weight=torch.zeros(10, 3, 1)),
        dict(background=torch.zeros(3)),                     # a batch needs (B, C)
        dict(background=torch.zeros(4, 2)),
        dict(background=torch.zeros(3, 4)),
        dict(points=torch.zeros(4, 10, 3)),                  # not (P, N_in)
        dict(points=torch.zeros(10, 2), point_weight=torch.zeros(10, 3)),  # N_in differs from rotation's columns
        dict(translation=torch.zeros(3, 2)),                 # B differs
        dict(rotation=torch.zeros(4, 3, 2), points=torch.zeros(10, 2), translation=torch.zeros(4, 3)),  # (2, 3)
        dict(rotation=torch.zeros(4, 1, 3), translation=torch.zeros(4, 1)),                              # (3, 1)
        dict(rotation=torch.zeros(4, 4), points=torch.zeros(10, 4), translation=torch.zeros(4)),         # (4, 4)
    ]
    for kw in bad:
        a = dict(points=pts, rotation=R, translation=t, point_weight=pw, background=None)
        a.update(kw)
        args = (a["points"], a["rotation"], a["translation"], a["point_weight"], a["background"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_channels((16, 16), *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_pullback_smooth_channels_(torch.zeros(16, 16, 3, 4), *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_channels_ad((16, 16), *args)
    # C = 0 and C = 17: libdpr's range, raised before any device is looked for
    for C in (0, 17):
        with pytest.raises(dpr_amd.DprError, match="out of range"):
            dpr_amd.raster_smooth_channels((16, 16), pts, R, t, torch.zeros(10, C))
        with pytest.raises(dpr_amd.DprError, match="out of range"):
            dpr_amd.raster_pullback_smooth_channels_(torch.zeros(16, 16, C, 4), pts, R, t, torch.zeros(10, C))
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.resolve_algo_smooth_channels("raster", (16, 16), 10, 4, 3, C)
    # consistent shapes on the CPU: there is no CPU path
    with pytest.raises(RuntimeError):
        dpr_amd.raster_smooth_channels((16, 16), pts, R, t, pw)
    # ... also with a ColumnMajorRotation, which is accepted wherever a rotation tensor is, and a background
    cm = dpr_amd.column_major_rotation(R)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster_smooth_channels((16, 16), pts, cm, t, pw, background=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster_pullback_smooth_channels_(torch.zeros(16, 16, 3, 4), pts, cm, t, pw, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster_smooth_channels((16, 16), pts, dpr_amd.column_major_rotation(R[0]), t[0], pw,
                                       background=torch.zeros(3))
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.raster_smooth_channels((16, 16), pts, cm, t, pw, background=torch.zeros(3))
    with pytest.raises(RuntimeError):
        dpr_amd.raster_pullback_smooth_channels_(torch.zeros(16, 16, 3, 4), pts, R, t, pw)
    # libdpr's own refusals come back as DprError
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes_smooth_channels("pullback", (16, 16), 10, 4, 3, 3, algo="tiled")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_channels("raster", (16, 16, 16), 10, 4, 2, 3)
