"""Host-side checks of the C ABI of the smooth splat of per-pose clouds (include/dpr.h, SMOOTH SPLAT, PER-POSE
CLOUDS): prototypes and exports, workspace sizes and the pose-group arithmetic, the AUTO rule against
tests/golden/smooth_clouds_auto.json, every refusal, and the Python shape checks.  No GPU needed: every refused call
returns before anything is launched."""
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
NEW = ["dpr_resolve_algo_smooth_clouds", "dpr_workspace_bytes_smooth_clouds_ex_f32",
       "dpr_workspace_bytes_smooth_clouds_ex_f64", "dpr_raster_smooth_clouds_ex_f32", "dpr_raster_smooth_clouds_ex_f64",
       "dpr_raster_pullback_smooth_clouds_ex_f32", "dpr_raster_pullback_smooth_clouds_ex_f64"]
PYTHON = ["raster_smooth_clouds", "raster_smooth_clouds_", "raster_pullback_smooth_clouds_", "raster_smooth_clouds_ad",
          "resolve_algo_smooth_clouds", "workspace_bytes_smooth_clouds"]
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
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in PYTHON:
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    assert L.dpr_version() == 110  # (no family after the ordered algorithm moved it)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes_smooth_clouds(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_smooth_clouds_ex_{suf}")
    single = getattr(L, f"dpr_workspace_bytes_smooth_ex_{suf}")
    dt = torch.float32 if suf == "f32" else torch.float64
    for n_in, n_out in PAIRS:
        grid = (37, 19, 21) if n_out == 3 else (150, 37)
        a, gp = _g(grid)
        # ATOMIC and P = 0: no workspace, either op, whatever the flags
        for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
            for fl in (0, _lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4)):
                assert f(op, _lib.ALGO_ATOMIC, fl, n_in, n_out, gp, 1000, 3) == 0
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 0, 3) == 0
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 0, 4) == 0
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1000, 0) != SIZE_MAX
        for P, B in ((1, 1), (1000, 7), (20_000, 16), (1_000_000, 40)):
            sizes = []
            for n in range(1, 17):
                need = f(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(n), n_in, n_out, gp, P, B)
                assert need != SIZE_MAX and need % 256 == 0
                # the single-pose layout for (group * tiles, group * P): what a pose of `group` clouds end to end needs
                bg = _group(grid, P, B, n)
                assert need >= 16 * bg * P + 4 * (bg * _tiles(grid) + 1)
                sizes.append(need)
            assert sizes == sorted(sizes), (P, B, sizes)  # monotone in max_pose_group
            default = f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, B)
            assert default >= sizes[-1] and default % 256 == 0
            assert default == f(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.FLAG_COHERENT_POINTS, n_in, n_out, gp, P, B)
            # a group of one: exactly the single-pose smooth workspace
            assert sizes[0] == single(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, 1)
            assert dpr_amd.workspace_bytes_smooth_clouds("raster", grid, P, B, n_in, dt, algo="tiled",
                                                         max_pose_group=1) \
                == dpr_amd.workspace_bytes_smooth("raster", grid, P, 1, n_in, dt, algo="tiled")
            if B == 1:
                assert default == sizes[0]
        # the refused combinations
        assert f(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1000, 3) == SIZE_MAX
        for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                assert f(op, algo, 0, n_in, n_out, gp, 1000, 3) == SIZE_MAX
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                assert f(op, _lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3) == SIZE_MAX
        assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3) == SIZE_MAX
        assert f(7, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, -1, 3) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, -1) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, None, 10, 1) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1 << 40, 1 << 19) == SIZE_MAX  # B P n_in > 2^60
        # TILED: P beyond 2^32 - 2 (a group of one: the limits of the single-pose tiled forward)
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 1, 1) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 2, 2) != SIZE_MAX
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1) == SIZE_MAX, (n_in, n_out)
    # the Python mirror
    assert dpr_amd.workspace_bytes_smooth_clouds("pullback", (16, 16), 10, 2, 3, algo="atomic") == 0
    assert dpr_amd.workspace_bytes_smooth_clouds("raster", (16, 16), 10, 2, 3, algo="tiled") > 160
    for op, algo in (("pullback", "tiled"), ("raster", "chunked"), ("raster", "ordered")):
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.workspace_bytes_smooth_clouds(op, (16, 16, 16), 10, 2, 3, algo=algo)
    with pytest.raises(KeyError):
        dpr_amd.workspace_bytes_smooth_clouds("residual_pullback", (16, 16), 10, 2, 3)
    with pytest.raises(ValueError):
        dpr_amd.workspace_bytes_smooth_clouds("raster", (16, 16), 10, 2, 3, algo="tiled", max_pose_group=17)


def test_default_group_is_cut_where_the_group_would_pass_two_to_the_24():
    """Host arithmetic only, on a grid of four tiles: two clouds of 2^23 points are one group (2^24 pairs), two of
    2^23 + 1 are two groups of one."""
    L = dpr_amd.lib()
    f = L.dpr_workspace_bytes_smooth_clouds_ex_f32
    single = L.dpr_workspace_bytes_smooth_ex_f32
    for n_in, n_out in PAIRS:
        grid = (20, 12, 9) if n_out == 3 else (70, 20)
        a, gp = _g(grid)
        P = 1 << 23
        cut = f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P + 1, 2)
        assert cut == single(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P + 1, 1)
        assert cut == f(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(1), n_in, n_out, gp, P + 1, 2)
        whole = f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, 2)
        assert whole > cut
        assert whole >= 16 * 2 * P
        assert whole > f(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(1), n_in, n_out, gp, P, 2)
        # more poses than a group holds change nothing: the workspace is reused from group to group
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, 4) == whole
    # a grid with more tiles than a cloud has points: the tiles bound the group
    a, gp = _g((512, 512, 512))
    tiles = _tiles((512, 512, 512))
    assert tiles == 32 * 64 * 64 and _group((512,) * 3, 1000, 1000) == GROUP_WORK // tiles
    by_tiles = f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp, 1000, 1000)
    assert by_tiles >= 4 * (128 * tiles + 1) and by_tiles < 4 * (129 * tiles + 1) + 40 * 128 * 1000 + (1 << 20)


def test_resolve_algo_smooth_clouds_matches_the_recorded_table():
    """AUTO on the probe's shapes (tests/golden/smooth_clouds_auto.json: the times profiles/smooth_clouds_probe.txt
    recorded, and the constants of the rule): within 1.15x of the faster forward on every row."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_clouds_auto.json")))
    L = dpr_amd.lib()
    names = {_lib.ALGO_ATOMIC: "atomic", _lib.ALGO_TILED: "tiled"}
    want_rows = {((128, 128), P, B) for P in (10**4, 10**5, 10**6) for B in (16, 64)} \
        | {((512, 512), P, 16) for P in (10**5, 10**6)} \
        | {((n, n, n), P, B) for n in (128, 256) for P in (10**5, 10**6) for B in (4, 16)}
    have = {(tuple(r["grid"]), r["P"], r["B"]) for r in table["shapes"]}
    assert want_rows <= have, want_rows - have
    min_work = table["constants"]["tiled_min_group_points"]
    per_tile = table["constants"]["tiled_min_points_per_tile"]
    assert table["constants"]["group_work"] == GROUP_WORK
    for row in table["shapes"]:
        grid = tuple(row["grid"])
        a, gp = _g(grid)
        n_out = len(grid)
        got = L.dpr_resolve_algo_smooth_clouds(_lib.OP_RASTER, row["n_in"], n_out, gp, row["P"], row["B"])
        assert got in names, (row, got)
        assert dpr_amd.resolve_algo_smooth_clouds("raster", grid, row["P"], row["B"], row["n_in"]) == names[got]
        # the rule as the table states it: TILED from min_work points in the default group on, for clouds of at
        # least per_tile points per tile of the grid
        bg = _group(grid, row["P"], row["B"])
        assert bg == row["group"]
        tiled = bg * row["P"] >= min_work[f"{n_out}d"] and row["P"] >= per_tile * _tiles(grid)
        assert names[got] == ("tiled" if tiled else "atomic"), row
        assert names[got] == row["auto"], row
        # the recorded times: AUTO within 1.15x of the faster forward
        t = {k: row["ms"][k] for k in ("atomic", "tiled")}
        assert t[names[got]] <= 1.15 * min(t.values()), (row, names[got])
        assert L.dpr_resolve_algo_smooth_clouds(_lib.OP_PULLBACK, row["n_in"], n_out, gp, row["P"], row["B"]) \
            == _lib.ALGO_ATOMIC
    # never CHUNKED or ORDERED, the pullback always ATOMIC, TILED only where the tiled forward can run
    for n_in, n_out in PAIRS:
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 10**4, 10**5, 10**6, 10**7, 10**9, (1 << 32) - 1):
                for B in (1, 16, 1000):
                    fw = L.dpr_resolve_algo_smooth_clouds(_lib.OP_RASTER, n_in, n_out, gp, P, B)
                    assert fw in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED), (grid, P, B, fw)
                    if fw == _lib.ALGO_TILED:
                        q = L.dpr_workspace_bytes_smooth_clouds_ex_f32(_lib.OP_RASTER, fw, 0, n_in, n_out, gp, P, B)
                        assert q != SIZE_MAX
                    assert L.dpr_resolve_algo_smooth_clouds(_lib.OP_PULLBACK, n_in, n_out, gp, P, B) \
                        == _lib.ALGO_ATOMIC
    a, gp = _g((64, 64))
    f = L.dpr_resolve_algo_smooth_clouds
    assert f(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2) == _lib.ERR_UNSUPPORTED_ALGO
    assert f(9, 3, 2, gp, 100, 2) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 0, 2, gp, 100, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(_lib.OP_RASTER, 2, 3, gp, 100, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(_lib.OP_RASTER, 2, 3, None, 100, 2) == _lib.ERR_UNSUPPORTED_DIMS  # (the grid is not looked at first)
    assert f(_lib.OP_RASTER, 3, 2, None, 100, 2) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 3, 2, gp, -1, 2) == _lib.ERR_INVALID_ARG
    assert f(_lib.OP_RASTER, 3, 2, gp, 1 << 40, 1 << 19) == _lib.ERR_INVALID_ARG


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    bad_grid, bgp = _g((16, 0, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_smooth_clouds_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_smooth_clouds_ex_{suf}")
        query = getattr(L, f"dpr_workspace_bytes_smooth_clouds_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, out=d, pts=d, rot=d, trans=d, grid=gp,
              ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, out, pts, rot, trans, None, None, None, ws, wsb)

        def b(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, g=d, pts=d, rot=d, trans=d,
              outs=(d, d, d, d, d, d), grid=gp, ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, grid, P, B, g, pts, rot, trans, None, None, *outs, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        # DPR_ERR_UNSUPPORTED_DIMS, before the grid is looked at
        for n_in, n_out in ALL_PAIRS:
            if (n_in, n_out) not in PAIRS:
                refused(f(n_in=n_in, n_out=n_out, grid=None), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
                refused(b(n_in=n_in, n_out=n_out, grid=None), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        refused(f(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        refused(b(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        # DPR_ERR_INVALID_ARG
        refused(f(out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        refused(f(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(f(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        assert f(grid=bgp) == _lib.ERR_INVALID_ARG and b(grid=bgp) == _lib.ERR_INVALID_ARG
        refused(f(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(P=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(b(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(out=odd), _lib.ERR_INVALID_ARG, "aligned")
        refused(f(P=1 << 40, B=1 << 19), _lib.ERR_INVALID_ARG, "too large")
        refused(b(P=1 << 40, B=1 << 19), _lib.ERR_INVALID_ARG, "too large")
        refused(b(g=None), _lib.ERR_INVALID_ARG, "ds_dout is NULL")
        refused(b(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(b(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(b(outs=(d, None, d, d, d, d)), _lib.ERR_INVALID_ARG, "per-pose output")
        refused(b(outs=(None, d, d, d, d, d)), _lib.ERR_INVALID_ARG, "ds_dpoints")
        refused(b(outs=(d, d, d, d, d, None)), _lib.ERR_INVALID_ARG, "ds_dpoint_weight")
        refused(b(outs=(d, d, odd, d, d, d)), _lib.ERR_INVALID_ARG, "aligned")
        for op in (7, -1):
            assert query(op, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 2) == SIZE_MAX
            assert "op" in _lib.last_error()
        # DPR_ERR_UNSUPPORTED_ALGO
        assert query(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, 3, 3, gp, 10, 2) == SIZE_MAX
        assert "residual" in _lib.last_error()
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            refused(f(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            refused(b(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            refused(f(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
            refused(b(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(b(algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "pullback runs on DPR_ALGO_ATOMIC only")
        refused(f(algo=_lib.ALGO_TILED, P=(1 << 32) - 1, B=1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")
        # DPR_ERR_WORKSPACE: none, one too small, one misaligned -- with the flags of the call in the query
        for fl in (0, _lib.flag_max_pose_group(1)):
            need = query(_lib.OP_RASTER, _lib.ALGO_TILED, fl, 3, 3, gp, 10, 2)
            refused(f(algo=_lib.ALGO_TILED, flags=fl), _lib.ERR_WORKSPACE, "workspace")
            refused(f(algo=_lib.ALGO_TILED, flags=fl, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
            refused(f(algo=_lib.ALGO_TILED, flags=fl, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        # the workspace of a group of one does not serve the default group
        one = query(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.flag_max_pose_group(1), 3, 3, gp, 1000, 2)
        refused(f(algo=_lib.ALGO_TILED, P=1000, ws=d, wsb=one), _lib.ERR_WORKSPACE, "workspace")
        # COHERENT_POINTS is accepted; B = 0: nothing to do, after the checks
        refused(f(flags=_lib.FLAG_COHERENT_POINTS, out=None), _lib.ERR_INVALID_ARG, "out is NULL")
        assert f(B=0) == _lib.OK and b(B=0) == _lib.OK
        refused(f(B=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")


def test_python_wrappers_raise_without_a_device():
    pts = torch.zeros(4, 10, 3)
    R, t = torch.zeros(4, 2, 3), torch.zeros(4, 2)
    bad = [
        dict(points=torch.zeros(10, 3)),                      # not (B, P, N_in)
        dict(points=torch.zeros(5, 10, 3)),                   # B differs from the poses'
        dict(rotation=torch.zeros(2, 3)),                     # an unbatched rotation
        dict(points=torch.zeros(4, 10, 2)),                   # N_in differs from rotation's columns
        dict(translation=torch.zeros(4, 3)),                  # N_out differs
        dict(translation=torch.zeros(3, 2)),                  # B differs
        dict(point_weight=torch.zeros(4, 9)),                 # neither (B, P) nor (P,)
        dict(rotation=torch.zeros(4, 3, 4), points=torch.zeros(4, 10, 4), translation=torch.zeros(4, 3)),  # (4, 3)
        dict(rotation=torch.zeros(4, 3, 2), points=torch.zeros(4, 10, 2), translation=torch.zeros(4, 3)),  # (2, 3)
        dict(rotation=torch.zeros(4, 1, 3), translation=torch.zeros(4, 1)),                                # (3, 1)
    ]
    for kw in bad:
        a = dict(points=pts, rotation=R, translation=t, point_weight=None)
        a.update(kw)
        args = (a["points"], a["rotation"], a["translation"], None, None, a["point_weight"])
        n_out = a["rotation"].shape[-2]
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_clouds((16,) * n_out, *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_pullback_smooth_clouds_(torch.zeros((16,) * n_out + (4,)), *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_clouds_ad((16,) * n_out, *args)
    # consistent shapes on the CPU: there is no CPU path
    with pytest.raises(RuntimeError):
        dpr_amd.raster_smooth_clouds((16, 16), pts, R, t)
    with pytest.raises(ValueError):
        dpr_amd.raster_smooth_clouds((16, 16), pts, R, t, max_pose_group=40)
    # libdpr's own refusals come back as DprError
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes_smooth_clouds("pullback", (16, 16), 10, 4, 3, algo="tiled")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_clouds("raster", (16, 16, 16), 10, 4, 2)
