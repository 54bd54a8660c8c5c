"""Host-side checks of the C ABI of the smooth splat of rigid bodies (include/dpr.h, SMOOTH SPLAT, RIGID BODIES):
prototypes and exports, workspace sizes and the group arithmetic, the AUTO rule against
tests/golden/smooth_bodies_auto.json, every refusal with its status, and the Python shape checks.  No GPU needed: every
refused call returns before anything is launched."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_resolve_algo_smooth_bodies", "dpr_workspace_bytes_smooth_bodies_ex_f32",
       "dpr_workspace_bytes_smooth_bodies_ex_f64", "dpr_raster_smooth_bodies_ex_f32", "dpr_raster_smooth_bodies_ex_f64",
       "dpr_raster_pullback_smooth_bodies_ex_f32", "dpr_raster_pullback_smooth_bodies_ex_f64"]
PYTHON = ["raster_smooth_bodies", "raster_smooth_bodies_", "raster_pullback_smooth_bodies_", "raster_smooth_bodies_ad",
          "resolve_algo_smooth_bodies"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
OPS = (_lib.OP_RASTER, _lib.OP_PULLBACK)
TILE = {2: (64, 16), 3: (16, 8, 8)}
GROUP_WORK = 1 << 24  # include/dpr.h, GROUP SIZE


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _tiles(grid):
    return int(np.prod([-(-n // e) for n, e in zip(grid, TILE[len(grid)])]))


def _group(grid, P, B, cap=0):
    bg = min(B, GROUP_WORK // max(P, _tiles(grid)))
    if cap:
        bg = min(bg, cap)
    return max(bg, 1)


def test_header_declares_and_library_exports_the_entry_points():
    raw = open(os.path.join(ROOT, "include", "dpr.h")).read()
    assert "SMOOTH SPLAT, RIGID BODIES" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in PYTHON:
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    assert L.dpr_version() == 110
    # `body` is const void *, K follows B: the argument lists of the dpr_*_bodies_ex_* prototypes
    for suf, t in (("f32", "float"), ("f64", "double")):
        for new, old in ((f"dpr_raster_smooth_bodies_ex_{suf}", f"dpr_raster_bodies_ex_{suf}"),
                         (f"dpr_raster_pullback_smooth_bodies_ex_{suf}", f"dpr_raster_pullback_bodies_ex_{suf}"),
                         (f"dpr_workspace_bytes_smooth_bodies_ex_{suf}", f"dpr_workspace_bytes_bodies_ex_{suf}")):
            proto = lambda n: re.sub(r"\s+", " ", re.search(rf"\b{n}\s*\((.*?)\)\s*;", text, flags=re.S).group(1))
            assert proto(new) == proto(old), new
    # no public query: tests/test_workspace_contract_table.py holds that list to its own table
    assert not any("bodies" in n for n in dir(dpr_amd) if n.startswith("workspace_bytes"))
    assert "no public workspace query" in sys.modules[dpr_amd.raster_smooth_bodies.__module__].__doc__


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_query(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_smooth_bodies_ex_{suf}")
    clouds = getattr(L, f"dpr_workspace_bytes_smooth_clouds_ex_{suf}")
    single = getattr(L, f"dpr_workspace_bytes_smooth_ex_{suf}")
    T = _lib.ALGO_TILED
    for n_in, n_out in PAIRS:
        grid = (37, 19, 21) if n_out == 3 else (150, 37)
        a, gp = _g(grid)
        # ATOMIC and P = 0: no workspace
        for op in OPS:
            for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC):
                for P, B, K in ((1000, 3, 4), (0, 3, 1), (1000, 0, 2), (0, 0, 1)):
                    assert f(op, algo, 0, n_in, n_out, gp, P, B, K) == 0, (op, algo, P, B, K)
                for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS):
                    assert f(op, algo, fl, n_in, n_out, gp, 1000, 3, 4) == 0
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, _lib.flag_max_pose_group(4), n_in, n_out, gp, 1000, 3, 4) == 0
        assert f(_lib.OP_RASTER, T, 0, n_in, n_out, gp, 0, 4, 3) == 0
        assert f(_lib.OP_RASTER, T, 0, n_in, n_out, gp, 1000, 0, 3) != SIZE_MAX
        # TILED: the smooth layout for (bg * tiles, bg * P) at groups of 1, 2 and the default, whatever K
        for P, B in ((1, 1), (1000, 7), (20_000, 16), (1_000_000, 40)):
            for K in (1, 5, 1 << 20):
                for cap in (1, 2, 0):
                    need = f(_lib.OP_RASTER, T, _lib.flag_max_pose_group(cap), n_in, n_out, gp, P, B, K)
                    assert need != SIZE_MAX and need % 256 == 0
                    bg = _group(grid, P, B, cap)
                    assert need >= 16 * bg * P + 4 * (bg * _tiles(grid) + 1)
                    # the layout arithmetic itself: that of the per-pose cloud family for the same (P, B), and for a
                    # whole number of groups that of the single-pose smooth forward on one (bg * tiles, bg * P) problem
                    assert need == clouds(_lib.OP_RASTER, T, _lib.flag_max_pose_group(cap), n_in, n_out, gp, P, B)
                    if bg == 1:
                        assert need == single(_lib.OP_RASTER, T, 0, n_in, n_out, gp, P, 1)
                assert f(_lib.OP_RASTER, T, 0, n_in, n_out, gp, P, B, K) \
                    == f(_lib.OP_RASTER, T, _lib.FLAG_COHERENT_POINTS, n_in, n_out, gp, P, B, K)
        # the layout arithmetic for (bg * tiles, bg * P), spelt out: a group of bg images of P points is one smooth
        # problem of bg * P points on a grid with bg times the tiles -- here `small` stacked bg times along its
        # last axis -- at groups of 1, 2 and the default (all 4 images)
        small = (60, 16, 8) if n_out == 3 else (64, 16)
        sa, sp = _g(small)
        for cap, bg in ((1, 1), (2, 2), (0, 4)):
            stacked = small[:-1] + (small[-1] * bg,)
            assert _tiles(stacked) == bg * _tiles(small) and _group(small, 5000, 4, cap) == bg
            xa, xp = _g(stacked)
            assert f(_lib.OP_RASTER, T, _lib.flag_max_pose_group(cap), n_in, n_out, sp, 5000, 4, 3) \
                == single(_lib.OP_RASTER, T, 0, n_in, n_out, xp, bg * 5000, 1)
        # the refused combinations
        for op in OPS:
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                assert f(op, _lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            for K in (0, -1):
                assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, K) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1, 1 << 31) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1 << 16, 1 << 15) == SIZE_MAX  # B * K = 2^31
            assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, (1 << 16) - 1, 1 << 15) == 0
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, -1, 3, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 10, -1, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, None, 10, 1, 4) == SIZE_MAX
        assert f(_lib.OP_PULLBACK, T, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        assert f(_lib.OP_PULLBACK, _lib.ALGO_ATOMIC, _lib.flag_max_pose_group(2), n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        assert f(7, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        # TILED where smooth_tile_count is 0: P beyond 2^32 - 2 (a group of one)
        assert f(_lib.OP_RASTER, T, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 2) == SIZE_MAX
        assert f(_lib.OP_RASTER, T, 0, n_in, n_out, gp, (1 << 32) - 2, 2, 2) != SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_AUTO, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 2) == 0  # AUTO: ATOMIC there
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 2) == SIZE_MAX, (n_in, n_out)


def test_resolve_algo_smooth_bodies_matches_the_recorded_table():
    """AUTO on the probe's rows (tests/golden/smooth_bodies_auto.json: the times profiles/smooth_bodies_probe.txt
    recorded, and the constants of the rule): within 1.15x of the faster forward on every row."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_bodies_auto.json")))
    L = dpr_amd.lib()
    names = {_lib.ALGO_ATOMIC: "atomic", _lib.ALGO_TILED: "tiled"}
    want_rows = {(grid, P, B, K, order)
                 for grid, P, B in (((512, 512), 10**6, 16), ((128, 128), 10**5, 64), ((128, 128, 128), 10**6, 4))
                 for K in (1, 4, 16, 64) for order in ("sorted", "shuffled")}
    have = {(tuple(r["grid"]), r["P"], r["B"], r["K"], r["order"]) for r in table["shapes"]}
    assert want_rows <= have, want_rows - have
    min_work = table["constants"]["tiled_min_group_points"]
    per_tile = table["constants"]["tiled_min_points_per_tile"]
    assert table["constants"]["group_work"] == GROUP_WORK and table["constants"]["margin"] == 1.15
    for row in table["shapes"]:
        grid = tuple(row["grid"])
        a, gp = _g(grid)
        n_out = len(grid)
        got = L.dpr_resolve_algo_smooth_bodies(_lib.OP_RASTER, row["n_in"], n_out, gp, row["P"], row["B"], row["K"])
        assert got in names, (row, got)
        assert dpr_amd.resolve_algo_smooth_bodies("raster", grid, row["P"], row["B"], row["K"], row["n_in"]) \
            == names[got]
        # the rule as the table states it: TILED from min_work (point, image) pairs in the default group on, for
        # clouds of at least per_tile points per tile of the grid; K does not enter
        bg = _group(grid, row["P"], row["B"])
        assert bg == row["group"]
        tiled = bg * row["P"] >= min_work[f"{n_out}d"] and row["P"] >= per_tile * _tiles(grid)
        assert names[got] == ("tiled" if tiled else "atomic"), row
        assert names[got] == row["auto"], row
        # the recorded times: AUTO within 1.15x of the faster forward
        t = {k: row["ms"][k] for k in ("atomic", "tiled")}
        assert t[names[got]] <= 1.15 * min(t.values()), (row, names[got])
        assert L.dpr_resolve_algo_smooth_bodies(_lib.OP_PULLBACK, row["n_in"], n_out, gp, row["P"], row["B"],
                                                row["K"]) == _lib.ALGO_ATOMIC
    # never CHUNKED or ORDERED, the pullback always ATOMIC, TILED only where the tiled forward can run
    f = L.dpr_resolve_algo_smooth_bodies
    for n_in, n_out in PAIRS:
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 10**4, 10**5, 10**6, 10**7, 10**9, (1 << 32) - 1):
                for B, K in ((1, 1), (16, 7), (1000, 1000)):
                    fw = f(_lib.OP_RASTER, n_in, n_out, gp, P, B, K)
                    assert fw in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED), (grid, P, B, K, fw)
                    tiles = _tiles(grid)
                    bg = _group(grid, P, B)
                    rule = P <= (1 << 32) - 2 and bg * P >= min_work[f"{n_out}d"] and P >= per_tile * tiles
                    assert (fw == _lib.ALGO_TILED) == rule, (grid, P, B, K)
                    if fw == _lib.ALGO_TILED:
                        q = L.dpr_workspace_bytes_smooth_bodies_ex_f32(_lib.OP_RASTER, fw, 0, n_in, n_out, gp, P, B, K)
                        assert q != SIZE_MAX
                    assert f(_lib.OP_PULLBACK, n_in, n_out, gp, P, B, K) == _lib.ALGO_ATOMIC
    a, gp = _g((64, 64))
    assert f(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_ALGO
    assert f(9, 3, 2, gp, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 0, 2, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(_lib.OP_RASTER, 2, 3, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(_lib.OP_RASTER, 2, 3, None, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS  # (the grid is not looked at first)
    assert f(_lib.OP_RASTER, 3, 2, None, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 3, 2, gp, 100, 2, 0) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 3, 2, gp, -1, 2, 2) == _lib.ERR_INVALID_ARG
    with pytest.raises(KeyError):
        dpr_amd.resolve_algo_smooth_bodies("residual_pullback", (64, 64), 100, 2, 2, 3)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_bodies("raster", (64, 64), 100, 2, 0, 3)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy aligned device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16, 16))
    bad_grid, bgp = _g((16, 0, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_smooth_bodies_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_smooth_bodies_ex_{suf}")
        query = getattr(L, f"dpr_workspace_bytes_smooth_bodies_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, out=d, pts=d, body=d, rot=d, trans=d,
              grid=gp, ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, K, out, pts, body, rot, trans, None, None, None,
                       ws, wsb)

        def b(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, g=d, pts=d, body=d, rot=d, trans=d,
              outs=(d, d, d, d, d, d), grid=gp, ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, grid, P, B, K, g, pts, body, rot, trans, None, None, *outs, ws,
                       wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        for call in (f, b):
            # DPR_ERR_UNSUPPORTED_DIMS: a pair other than the three, before the grid is looked at
            refused(call(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
            refused(call(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
            for n_in, n_out in ALL_PAIRS:
                if (n_in, n_out) not in PAIRS:
                    refused(call(n_in=n_in, n_out=n_out, grid=None), _lib.ERR_UNSUPPORTED_DIMS,
                            "supports (2,2), (3,3), (3,2)")
            # DPR_ERR_INVALID_ARG: K < 1, B * K beyond the range the kernels index with, sizes, pointers
            refused(call(K=0), _lib.ERR_INVALID_ARG, "at least one body")
            refused(call(K=-3), _lib.ERR_INVALID_ARG, "at least one body")
            refused(call(B=1 << 16, K=1 << 15), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
            refused(call(B=1, K=1 << 31), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
            refused(call(B=-1), _lib.ERR_INVALID_ARG, "negative")
            refused(call(P=-1), _lib.ERR_INVALID_ARG, "negative")
            refused(call(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
            assert call(grid=bgp) == _lib.ERR_INVALID_ARG
            refused(call(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
            refused(call(body=None), _lib.ERR_INVALID_ARG, "body is NULL")
            refused(call(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
            refused(call(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
            refused(call(pts=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(rot=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(body=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(ws=odd, wsb=1024), _lib.ERR_WORKSPACE, "256-byte aligned")
            # DPR_ERR_UNSUPPORTED_ALGO: CHUNKED / ORDERED / unknown, KEEP / REUSE
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                refused(call(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                refused(call(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            # refusals come before the empty-batch return
            refused(call(B=0, P=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
            refused(call(B=0, P=0, K=0), _lib.ERR_INVALID_ARG, "at least one body")
            # P = 0 and B = 0 together: valid, empty, nothing to launch; COHERENT_POINTS is accepted
            assert call(B=0, P=0) == _lib.OK
            assert call(B=0, P=0, flags=_lib.FLAG_COHERENT_POINTS) == _lib.OK
        # the residual pullback and a bad op (the query carries the op)
        assert query(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 2, 3) == SIZE_MAX
        assert "residual" in _lib.last_error()
        for op in (7, -1):
            assert query(op, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 2, 3) == SIZE_MAX
            assert "op" in _lib.last_error()
        # DPR_ALGO_TILED: refused for the pullback, and for the forward where smooth_tile_count is 0
        refused(b(algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "pullback runs on DPR_ALGO_ATOMIC only")
        refused(b(algo=_lib.ALGO_TILED, B=0, P=0), _lib.ERR_UNSUPPORTED_ALGO, "pullback runs on DPR_ALGO_ATOMIC only")
        refused(f(algo=_lib.ALGO_TILED, P=(1 << 32) - 1, B=1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")
        # DPR_FLAG_MAX_POSE_GROUP: accepted on the forward (either algorithm), refused on the pullback
        refused(b(flags=_lib.flag_max_pose_group(4)), _lib.ERR_UNSUPPORTED_ALGO, "DPR_FLAG_MAX_POSE_GROUP")
        refused(f(flags=_lib.flag_max_pose_group(4), out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        assert f(flags=_lib.flag_max_pose_group(4), B=0) == _lib.OK
        # DPR_ERR_WORKSPACE: none, one too small, one misaligned -- with the flags of the call in the query
        for fl in (0, _lib.flag_max_pose_group(1)):
            need = query(_lib.OP_RASTER, _lib.ALGO_TILED, fl, 3, 3, gp, 10, 2, 3)
            assert need not in (0, SIZE_MAX)
            refused(f(algo=_lib.ALGO_TILED, flags=fl), _lib.ERR_WORKSPACE, "workspace")
            refused(f(algo=_lib.ALGO_TILED, flags=fl, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
            refused(f(algo=_lib.ALGO_TILED, flags=fl, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        # the workspace of a group of one does not serve the default group
        one = query(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(1), 3, 3, gp, 1000, 2, 3)
        refused(f(algo=_lib.ALGO_TILED, P=1000, ws=d, wsb=one), _lib.ERR_WORKSPACE, "workspace")
        refused(f(out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        refused(f(out=odd), _lib.ERR_INVALID_ARG, "aligned")
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
            dpr_amd.raster_smooth_bodies((16, 16), *args, point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_pullback_smooth_bodies_(torch.zeros(16, 16, 4), *args, point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_bodies_ad((16, 16), *args, point_weight=a["point_weight"])
    with pytest.raises(TypeError):
        dpr_amd.raster_smooth_bodies((16, 16), pts, body.float(), R, t)
    with pytest.raises(ValueError):
        dpr_amd.raster_smooth_bodies((16, 16), pts, body, R, t, max_pose_group=40)
    # consistent shapes on the CPU: the error of `raster`
    for call in (lambda: dpr_amd.raster_smooth_bodies((16, 16), pts, body, R, t),
                 lambda: dpr_amd.raster_smooth_bodies((16, 16), pts, body, R[0], t[0]),
                 lambda: dpr_amd.raster_smooth_bodies_(torch.zeros(16, 16, 4), pts, body, R, t),
                 lambda: dpr_amd.raster_pullback_smooth_bodies_(torch.zeros(16, 16, 4), pts, body, R, t),
                 lambda: dpr_amd.raster_smooth_bodies_ad((16, 16), pts, body, R, t)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
