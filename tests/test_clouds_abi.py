"""Host-side checks of the per-pose cloud C ABI (include/dpr.h, PER-POSE CLOUDS): prototypes and exports, workspace
sizes, the AUTO rule against tests/golden/clouds_auto.json, argument errors and the Python shape checks.  No GPU
needed: every refused call returns before anything is launched."""
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
NEW = ["dpr_raster_clouds_ex_f32", "dpr_raster_clouds_ex_f64", "dpr_raster_pullback_clouds_ex_f32",
       "dpr_raster_pullback_clouds_ex_f64", "dpr_workspace_bytes_clouds_ex_f32", "dpr_workspace_bytes_clouds_ex_f64",
       "dpr_resolve_algo_clouds"]
SIZE_MAX = ctypes.c_size_t(-1).value
PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
ALL_ALGO_PAIRS = [(2, 2), (3, 3), (3, 2)]


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_cloud_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert L.dpr_version() >= 109
    for name in ("raster_clouds", "raster_clouds_", "raster_pullback_clouds_", "raster_clouds_ad",
                 "resolve_algo_clouds", "workspace_bytes_clouds"):
        assert callable(getattr(dpr_amd, name)), name


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes_clouds(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_clouds_ex_{suf}")
    single = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
        for n_in, n_out in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3) == 0, (op, n_in, n_out)
            # flags that keep their meaning or are ignored
            for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4)):
                assert f(op, _lib.ALGO_ATOMIC, fl, n_in, n_out, gp, 1000, 3) == 0
        # TILED: the single-pose tiled workspace, whatever B
        for grid, n_in in (((256, 256, 256), 3), ((512, 512), 3), ((512, 512), 2)):
            a, gp = _g(grid)
            ref = single(op, _lib.ALGO_TILED, 0, n_in, len(grid), gp, 2_000_000, 1)
            assert ref not in (0, SIZE_MAX)
            for B in (1, 4, 64):
                assert f(op, _lib.ALGO_TILED, 0, n_in, len(grid), gp, 2_000_000, B) == ref
        # CHUNKED: a valid size for every pair that has it
        for (n_in, n_out) in ALL_ALGO_PAIRS:
            a, gp = _g((200, 150) if n_out == 2 else (40, 33, 20))
            assert f(op, _lib.ALGO_CHUNKED, 0, n_in, n_out, gp, 20000, 7) != SIZE_MAX
    # refused: bad dims and grids, negative sizes, the residual op, unknown ops, KEEP / REUSE, TILED / CHUNKED on
    # pairs without them
    a, gp = _g((16, 16, 16))
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 5, 3, gp, 10, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 0, gp, 10, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, -1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 3, gp, -1, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 3, None, 10, 1) == SIZE_MAX
    assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 1) == SIZE_MAX
    assert f(7, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 1) == SIZE_MAX
    for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
        assert f(_lib.OP_RASTER, _lib.ALGO_AUTO, fl, 3, 3, gp, 10, 1) == SIZE_MAX
    for n_in, n_out in PAIRS:
        if (n_in, n_out) in ALL_ALGO_PAIRS:
            continue
        a, gp = _g((16,) * n_out)
        for algo in (_lib.ALGO_TILED, _lib.ALGO_CHUNKED):
            assert f(_lib.OP_RASTER, algo, 0, n_in, n_out, gp, 10, 1) == SIZE_MAX, (n_in, n_out)
    # 64-bit sizes: B * P * n_in beyond 2^60
    a, gp = _g((16, 16))
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 2, gp, 1 << 40, 1 << 20) == SIZE_MAX
    # the Python mirror
    assert dpr_amd.workspace_bytes_clouds("raster", (16, 16), 10, 2, 3, algo="atomic") == 0
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes_clouds("raster", (16, 16, 16), 10, 2, 2, algo="chunked")


def test_resolve_algo_clouds_matches_the_recorded_table():
    """AUTO on the probe shapes and around its thresholds (tests/golden/clouds_auto.json: the choices, and the times
    profiles/clouds_probe.txt recorded for them)."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "clouds_auto.json")))
    L = dpr_amd.lib()
    for row in table["shapes"]:
        a, gp = _g(row["grid"])
        dtype = getattr(torch, row.get("dtype", "float32"))
        for op, want in row["auto"].items():
            opc = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}[op]
            if dtype == torch.float32:  # (the C query answers for fp32 data)
                got = L.dpr_resolve_algo_clouds(opc, row["n_in"], len(row["grid"]), gp, row["P"], row["B"])
                assert got == _lib.ALGOS[want], (row, op)
            assert dpr_amd.resolve_algo_clouds(op, row["grid"], row["P"], row["B"], row["n_in"], dtype) == want
            # the recorded times: AUTO within 1.15x of the fastest algorithm of the family
            t = row["ms"][op]
            best = min(v for k, v in t.items() if k in ("atomic", "tiled", "chunked") and v is not None)
            assert t[want] <= 1.15 * best, (row["name"], op)
    # pairs without the tiled / chunked paths: always ATOMIC
    for n_in, n_out in PAIRS:
        if (n_in, n_out) not in ALL_ALGO_PAIRS:
            a, gp = _g((64,) * n_out)
            assert L.dpr_resolve_algo_clouds(_lib.OP_RASTER, n_in, n_out, gp, 10_000, 8) == _lib.ALGO_ATOMIC
    a, gp = _g((64, 64))
    assert L.dpr_resolve_algo_clouds(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2) == _lib.ERR_UNSUPPORTED_ALGO
    assert L.dpr_resolve_algo_clouds(9, 3, 2, gp, 100, 2) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_clouds(_lib.OP_RASTER, 0, 2, gp, 100, 2) == _lib.ERR_UNSUPPORTED_DIMS


def test_cloud_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16, 16))  # (four sizes: the (4, 4) pair below reads grid[3]; n_out = 3 reads the first three)
    d = ctypes.c_void_p(256)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_clouds_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_clouds_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, out=d, pts=d, rot=d, trans=d, grid=gp,
              ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, out, pts, rot, trans, None, None, None, ws, wsb)

        def b(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, g=d, pts=d, rot=d, trans=d,
              outs=(d, d, d, d, d, d), ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, gp, P, B, g, pts, rot, trans, None, None, *outs, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        refused(f(out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        refused(f(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(f(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        refused(f(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        refused(f(flags=_lib.FLAG_KEEP_BINNING), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        refused(f(flags=_lib.FLAG_REUSE_BINNING), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        refused(f(algo=9), _lib.ERR_UNSUPPORTED_ALGO, "unknown algorithm")
        refused(f(P=1 << 40, B=1 << 20), _lib.ERR_INVALID_ARG, "too large")
        if suf == "f32":  # (the fp32 forward keeps its per-pose weight ranges in the workspace)
            refused(f(algo=_lib.ALGO_CHUNKED), _lib.ERR_WORKSPACE, "workspace")
        for n_in, n_out in ((2, 3), (4, 4), (1, 1), (2, 1)):
            for algo in (_lib.ALGO_TILED, _lib.ALGO_CHUNKED):
                refused(f(algo=algo, n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_ALGO, "ATOMIC only")
                refused(b(algo=algo, n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_ALGO, "ATOMIC only")
        refused(b(g=None), _lib.ERR_INVALID_ARG, "ds_dout is NULL")
        refused(b(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(b(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(b(outs=(d, None, d, d, d, d)), _lib.ERR_INVALID_ARG, "per-pose output")
        refused(b(outs=(None, d, d, d, d, d)), _lib.ERR_INVALID_ARG, "ds_dpoints")
        refused(b(outs=(d, d, d, d, d, None)), _lib.ERR_INVALID_ARG, "ds_dpoint_weight")
        refused(b(flags=_lib.FLAG_KEEP_BINNING), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        refused(b(algo=_lib.ALGO_CHUNKED), _lib.ERR_WORKSPACE, "workspace")
        refused(b(algo=_lib.ALGO_TILED), _lib.ERR_WORKSPACE, "workspace")
        refused(b(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        # the residual op has no per-pose cloud variant
        g2, gp2 = _g((16, 16))
        assert L.dpr_resolve_algo_clouds(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp2, 10, 2) == _lib.ERR_UNSUPPORTED_ALGO


def test_python_wrappers_raise_dimension_mismatch_before_any_library_call():
    pts = torch.zeros(4, 10, 3)
    R, t = torch.zeros(4, 2, 3), torch.zeros(4, 2)
    bad = [
        dict(points=torch.zeros(10, 3)),                     # not (B, P, N_in)
        dict(points=torch.zeros(5, 10, 3)),                  # B differs from the poses
        dict(points=torch.zeros(4, 10, 2)),                  # N_in differs from rotation's columns
        dict(rotation=torch.zeros(2, 3)),                    # unbatched pose
        dict(translation=torch.zeros(4, 3)),                 # N_out differs
        dict(translation=torch.zeros(3, 2)),                 # B differs
        dict(point_weight=torch.ones(4, 9)),                 # P differs
        dict(point_weight=torch.ones(9)),
        dict(point_weight=torch.ones(3, 10)),                # B differs
    ]
    for kw in bad:
        a = dict(points=pts, rotation=R, translation=t, point_weight=None)
        a.update(kw)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_clouds((16, 16), a["points"], a["rotation"], a["translation"],
                                  point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_pullback_clouds_(torch.zeros(16, 16, 4), a["points"], a["rotation"], a["translation"],
                                            point_weight=a["point_weight"])
    # consistent shapes on the CPU: there is no CPU path
    with pytest.raises(RuntimeError):
        dpr_amd.raster_clouds((16, 16), pts, R, t, point_weight=torch.ones(10))
