"""Host-side checks of the C ABI of the forward mode of the smooth splat of rigid bodies (include/dpr.h, SMOOTH SPLAT,
RIGID BODIES, FORWARD MODE): prototypes and exports, the workspace query against the forward's, the AUTO rule against
tests/golden/smooth_bodies_jvp_auto.json, every refusal with its status, and the Python shape checks.  No GPU needed:
every refused call returns before anything is launched."""
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
NEW = ["dpr_resolve_algo_smooth_bodies_jvp", "dpr_workspace_bytes_smooth_bodies_jvp_ex_f32",
       "dpr_workspace_bytes_smooth_bodies_jvp_ex_f64", "dpr_raster_smooth_bodies_jvp_ex_f32",
       "dpr_raster_smooth_bodies_jvp_ex_f64"]
PYTHON = ["raster_smooth_bodies_jvp", "raster_smooth_bodies_jvp_", "resolve_algo_smooth_bodies_jvp"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
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
    assert "SMOOTH SPLAT, RIGID BODIES, FORWARD MODE" in raw
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
    proto = lambda n: re.sub(r"\s+", " ", re.search(rf"\b{n}\s*\((.*?)\)\s*;", text, flags=re.S).group(1))
    for suf, t in (("f32", "float"), ("f64", "double")):
        # the argument list of dpr_raster_smooth_jvp_ex_* with `body` (const void *) behind points and V behind K
        want = proto(f"dpr_raster_smooth_jvp_ex_{suf}").replace("int64_t K,", "int64_t K, int64_t V,") \
            .replace(f"const {t} *points,", f"const {t} *points, const void *body,")
        assert proto(f"dpr_raster_smooth_bodies_jvp_ex_{suf}") == want
        assert proto(f"dpr_workspace_bytes_smooth_bodies_jvp_ex_{suf}") \
            == proto(f"dpr_workspace_bytes_smooth_jvp_ex_{suf}") + ", int64_t V"
    assert proto("dpr_resolve_algo_smooth_bodies_jvp") == proto("dpr_resolve_algo_smooth_jvp") + ", int64_t V"
    # no public query: tests/test_workspace_contract_table.py holds that list to its own table
    assert not any("bodies" in n for n in dir(dpr_amd) if n.startswith("workspace_bytes"))
    assert "no public workspace query" in sys.modules[dpr_amd.raster_smooth_bodies_jvp.__module__].__doc__


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_query(suf):
    """Exactly the forward's workspace for the same (grid, P, B, flags), whatever K and V; 0 for ATOMIC and P = 0."""
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_smooth_bodies_jvp_ex_{suf}")
    fwd = getattr(L, f"dpr_workspace_bytes_smooth_bodies_ex_{suf}")
    T = _lib.ALGO_TILED
    for n_in, n_out in PAIRS:
        grid = (37, 19, 21) if n_out == 3 else (150, 37)
        a, gp = _g(grid)
        for P, B, K in ((1000, 3, 4), (0, 3, 1), (1000, 0, 2), (0, 0, 1)):
            for V in (1, 5, 16):
                assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, P, B, K, V) == 0, (P, B, K, V)
                # AUTO: 0 where it resolves to ATOMIC, the TILED bytes where it resolves to TILED
                auto = L.dpr_resolve_algo_smooth_bodies_jvp(n_in, n_out, gp, P, B, K, V)
                assert auto in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)
                assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, P, B, K, V) == f(auto, 0, n_in, n_out, gp, P, B, K, V)
                if P == 0 or V == 1:  # (no work, or too little for the binning to pay)
                    assert auto == _lib.ALGO_ATOMIC and f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, P, B, K, V) == 0
        for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4)):
            assert f(_lib.ALGO_ATOMIC, fl, n_in, n_out, gp, 1000, 3, 4, 2) == 0
            assert f(_lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, 4, 1) == 0
        assert f(T, 0, n_in, n_out, gp, 0, 4, 3, 2) == 0
        assert f(T, 0, n_in, n_out, gp, 1000, 0, 3, 2) != SIZE_MAX
        for P, B in ((1, 1), (1000, 7), (20_000, 16), (1_000_000, 40)):
            for K in (1, 5, 1 << 20):
                for V in (1, 5, 16):
                    for cap in (1, 2, 0):
                        fl = _lib.flag_max_pose_group(cap)
                        need = f(T, fl, n_in, n_out, gp, P, B, K, V)
                        assert need not in (0, SIZE_MAX) and need % 256 == 0
                        assert need == fwd(_lib.OP_RASTER, T, fl, n_in, n_out, gp, P, B, K), (P, B, K, V, cap)
                        bg = _group(grid, P, B, cap)
                        assert need >= 16 * bg * P + 4 * (bg * _tiles(grid) + 1)
        # AUTO where it resolves to TILED: the same bytes
        big = f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 1_000_000, 4, 3, 2)
        assert big == f(T, 0, n_in, n_out, gp, 1_000_000, 4, 3, 2) > 0
        # the refused combinations
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            assert f(algo, 0, n_in, n_out, gp, 1000, 3, 4, 2) == SIZE_MAX
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            assert f(_lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, 4, 2) == SIZE_MAX
        for K in (0, -1):
            assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, K, 2) == SIZE_MAX
        for V in (0, -1, 17):
            assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, 4, V) == SIZE_MAX
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1, 1 << 31, 2) == SIZE_MAX
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1 << 16, 1 << 15, 2) == SIZE_MAX  # B * K = 2^31
        assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, (1 << 16) - 1, 1 << 15, 2) == 0
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, -1, 3, 4, 2) == SIZE_MAX
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 10, -1, 4, 2) == SIZE_MAX
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, None, 10, 1, 4, 2) == SIZE_MAX
        # TILED where smooth_tile_count is 0: P beyond 2^32 - 2 (a group of one)
        assert f(T, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 2, 2) == SIZE_MAX
        assert f(T, 0, n_in, n_out, gp, (1 << 32) - 2, 2, 2, 2) != SIZE_MAX
        assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 2, 2) == 0  # AUTO: ATOMIC there
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 2, 1) == SIZE_MAX, (n_in, n_out)


def test_resolve_algo_smooth_bodies_jvp_matches_the_recorded_table():
    """AUTO on the probe's rows (tests/golden/smooth_bodies_jvp_auto.json: the times
    profiles/smooth_bodies_jvp_probe.txt recorded, and the constants of the rule): within 1.15x of the faster of
    ATOMIC and TILED on every row."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_bodies_jvp_auto.json")))
    L = dpr_amd.lib()
    names = {_lib.ALGO_ATOMIC: "atomic", _lib.ALGO_TILED: "tiled"}
    want_rows = {(grid, P, B, K, V, order)
                 for grid, P, B in (((512, 512), 10**6, 16), ((128, 128), 10**5, 64), ((128, 128, 128), 10**6, 4))
                 for K in (1, 4, 64) for V in (1, 12) for order in ("sorted", "shuffled")}
    have = {(tuple(r["grid"]), r["P"], r["B"], r["K"], r["V"], r["order"]) for r in table["shapes"]}
    assert want_rows <= have, want_rows - have
    min_work = table["constants"]["tiled_min_group_work"]
    per_tile = table["constants"]["tiled_min_points_per_tile"]
    assert table["constants"]["group_work"] == GROUP_WORK and table["constants"]["margin"] == 1.15
    for row in table["shapes"]:
        grid = tuple(row["grid"])
        a, gp = _g(grid)
        n_out = len(grid)
        got = L.dpr_resolve_algo_smooth_bodies_jvp(row["n_in"], n_out, gp, row["P"], row["B"], row["K"], row["V"])
        assert got in names, (row, got)
        assert dpr_amd.resolve_algo_smooth_bodies_jvp(grid, row["P"], row["B"], row["K"], row["n_in"], row["V"]) \
            == names[got]
        # the rule as the table states it: TILED where the default group holds bg * P * V^2 >= min_work, for clouds of
        # at least per_tile points per tile of the grid; K does not enter
        bg = _group(grid, row["P"], row["B"])
        assert bg == row["group"]
        tiled = bg * row["P"] * row["V"] ** 2 >= min_work[f"{n_out}d"] and row["P"] >= per_tile * _tiles(grid)
        assert names[got] == ("tiled" if tiled else "atomic"), row
        assert names[got] == row["auto"], row
        t = {k: row["ms"][k] for k in ("atomic", "tiled")}
        assert t[names[got]] <= 1.15 * min(t.values()), (row, names[got])
    # never CHUNKED or ORDERED, TILED only where the tiled path can run
    f = L.dpr_resolve_algo_smooth_bodies_jvp
    for n_in, n_out in PAIRS:
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 10**4, 10**5, 10**6, 10**7, 10**9, (1 << 32) - 1):
                for B, K in ((1, 1), (16, 7), (1000, 1000)):
                    for V in (1, 3, 16):
                        got = f(n_in, n_out, gp, P, B, K, V)
                        assert got in names, (grid, P, B, K, V, got)
                        bg = _group(grid, P, B)
                        rule = (P <= (1 << 32) - 2 and bg * P * V * V >= min_work[f"{n_out}d"]
                                and P >= per_tile * _tiles(grid))
                        assert (got == _lib.ALGO_TILED) == rule, (grid, P, B, K, V)
                        if got == _lib.ALGO_TILED:
                            q = L.dpr_workspace_bytes_smooth_bodies_jvp_ex_f32(got, 0, n_in, n_out, gp, P, B, K, V)
                            assert q != SIZE_MAX
    a, gp = _g((64, 64))
    assert f(0, 2, gp, 100, 2, 2, 1) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(2, 3, gp, 100, 2, 2, 1) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(2, 3, None, 100, 2, 2, 1) == _lib.ERR_UNSUPPORTED_DIMS  # (the grid is not looked at first)
    assert f(3, 2, None, 100, 2, 2, 1) == _lib.ERR_INVALID_ARG
    assert f(3, 2, gp, 100, 2, 0, 1) == _lib.ERR_INVALID_ARG
    assert f(3, 2, gp, 100, 2, 2, 0) == _lib.ERR_INVALID_ARG
    assert f(3, 2, gp, 100, 2, 2, 17) == _lib.ERR_INVALID_ARG
    assert f(3, 2, gp, -1, 2, 2, 1) == _lib.ERR_INVALID_ARG
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_bodies_jvp((64, 64), 100, 2, 0, 3)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_bodies_jvp((64, 64), 100, 2, 2, 3, tangents=17)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy aligned device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16, 16))
    bad_grid, bgp = _g((16, 0, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        entry = getattr(L, f"dpr_raster_smooth_bodies_jvp_ex_{suf}")
        query = getattr(L, f"dpr_workspace_bytes_smooth_bodies_jvp_ex_{suf}")

        def call(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, V=2, out=d, pts=d, body=d, rot=d,
                 trans=d, tans=(d, None, None, None, None, None), grid=gp, ws=None, wsb=0):
            return entry(None, algo, flags, n_in, n_out, grid, P, B, K, V, out, pts, body, rot, trans, None, None,
                         *tans, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        # DPR_ERR_UNSUPPORTED_DIMS: a pair other than the three, before the grid is looked at
        refused(call(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        refused(call(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        for n_in, n_out in ALL_PAIRS:
            if (n_in, n_out) not in PAIRS:
                refused(call(n_in=n_in, n_out=n_out, grid=None), _lib.ERR_UNSUPPORTED_DIMS,
                        "supports (2,2), (3,3), (3,2)")
        # DPR_ERR_INVALID_ARG: K < 1, B * K, V outside 1..16, sizes, pointers
        refused(call(K=0), _lib.ERR_INVALID_ARG, "at least one body")
        refused(call(K=-3), _lib.ERR_INVALID_ARG, "at least one body")
        refused(call(B=1 << 16, K=1 << 15), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
        refused(call(B=1, K=1 << 31), _lib.ERR_INVALID_ARG, "exceed 2^31 - 1")
        refused(call(V=0), _lib.ERR_INVALID_ARG, "out of range [1, 16]")
        refused(call(V=17), _lib.ERR_INVALID_ARG, "out of range [1, 16]")
        refused(call(V=-1), _lib.ERR_INVALID_ARG, "out of range [1, 16]")
        refused(call(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(call(P=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(call(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        assert call(grid=bgp) == _lib.ERR_INVALID_ARG
        refused(call(out=None), _lib.ERR_INVALID_ARG, "out_dot is NULL")
        refused(call(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(call(body=None), _lib.ERR_INVALID_ARG, "body is NULL")
        refused(call(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(call(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        for bad in ("out", "pts", "rot", "trans"):
            refused(call(**{bad: odd}), _lib.ERR_INVALID_ARG, "aligned")
        refused(call(body=odd), _lib.ERR_INVALID_ARG, "aligned")
        for i in range(6):  # every tangent pointer is checked
            tans = [None] * 6
            tans[i] = odd
            refused(call(tans=tuple(tans)), _lib.ERR_INVALID_ARG, "aligned")
        refused(call(ws=odd, wsb=1024), _lib.ERR_WORKSPACE, "256-byte aligned")
        # DPR_ERR_UNSUPPORTED_ALGO: CHUNKED / ORDERED / unknown, KEEP / REUSE
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            refused(call(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
            assert query(algo, 0, 3, 3, gp, 10, 2, 3, 2) == SIZE_MAX
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING, 3):
            refused(call(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            refused(call(flags=fl, algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            assert query(_lib.ALGO_TILED, fl, 3, 3, gp, 10, 2, 3, 2) == SIZE_MAX
        refused(call(algo=_lib.ALGO_TILED, P=(1 << 32) - 1, B=1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")
        # refusals come before the empty-batch return
        refused(call(B=0, P=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(call(B=0, P=0, K=0), _lib.ERR_INVALID_ARG, "at least one body")
        refused(call(B=0, P=0, V=17), _lib.ERR_INVALID_ARG, "out of range")
        # B = 0: valid, nothing to do; the other flags are accepted
        assert call(B=0, P=0) == _lib.OK
        assert call(B=0, flags=_lib.FLAG_COHERENT_POINTS | _lib.flag_max_pose_group(4)) == _lib.OK
        assert call(B=0, pts=None, body=None, rot=None, trans=None, out=None) == _lib.OK
        # DPR_ERR_WORKSPACE: none, one too small, one misaligned -- with the flags of the call in the query
        for fl in (0, _lib.flag_max_pose_group(1)):
            need = query(_lib.ALGO_TILED, fl, 3, 3, gp, 10, 2, 3, 2)
            assert need not in (0, SIZE_MAX)
            refused(call(algo=_lib.ALGO_TILED, flags=fl), _lib.ERR_WORKSPACE, "workspace")
            refused(call(algo=_lib.ALGO_TILED, flags=fl, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
            refused(call(algo=_lib.ALGO_TILED, flags=fl, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        # the workspace of a group of one does not serve the default group
        one = query(_lib.ALGO_TILED, _lib.flag_max_pose_group(1), 3, 3, gp, 1000, 2, 3, 2)
        refused(call(algo=_lib.ALGO_TILED, P=1000, ws=d, wsb=one), _lib.ERR_WORKSPACE, "workspace")


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
            dpr_amd.raster_smooth_bodies_jvp((16, 16), *args, point_weight=a["point_weight"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_bodies_jvp_(torch.zeros(16, 16, 2, 4), *args, point_weight=a["point_weight"],
                                              tangents=2)
    with pytest.raises(TypeError):
        dpr_amd.raster_smooth_bodies_jvp((16, 16), pts, body.float(), R, t)
    with pytest.raises(ValueError):
        dpr_amd.raster_smooth_bodies_jvp((16, 16), pts, body, R, t, max_pose_group=40)
    for tangents in (0, 17, True, 2.0):  # V outside 1..16, before anything else
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.raster_smooth_bodies_jvp((16, 16), pts, body, R, t, tangents=tangents)
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.raster_smooth_bodies_jvp_(torch.zeros(16, 16, 4), pts, body, R, t, tangents=tangents)
    # consistent shapes on the CPU: the error of `raster`
    for call in (lambda: dpr_amd.raster_smooth_bodies_jvp((16, 16), pts, body, R, t),
                 lambda: dpr_amd.raster_smooth_bodies_jvp((16, 16), pts, body, R[0], t[0], tangents=3),
                 lambda: dpr_amd.raster_smooth_bodies_jvp_(torch.zeros(16, 16, 4), pts, body, R, t)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
