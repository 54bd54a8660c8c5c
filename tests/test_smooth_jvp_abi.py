"""Host-side checks of the smooth splat's forward-mode C ABI (include/dpr.h, SMOOTH SPLAT, FORWARD MODE): prototypes
and exports, workspace sizes, the AUTO rule against tests/golden/smooth_jvp_auto.json, every refusal, and the Python
shape checks.  No GPU needed: every refused call returns before anything is launched."""
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
NEW = ["dpr_resolve_algo_smooth_jvp", "dpr_workspace_bytes_smooth_jvp_ex_f32", "dpr_workspace_bytes_smooth_jvp_ex_f64",
       "dpr_raster_smooth_jvp_ex_f32", "dpr_raster_smooth_jvp_ex_f64"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
GRIDS = {2: (150, 37), 3: (37, 19, 21)}


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
    # exactly the argument list of dpr_raster_jvp_ex_*
    for suf in ("f32", "f64"):
        args = lambda n: re.sub(r"\s+", " ", re.search(rf"\b{n}_{suf}\s*\((.*?)\)", text, flags=re.S).group(1))
        assert args("dpr_raster_smooth_jvp_ex") == args("dpr_raster_jvp_ex")
        assert args("dpr_workspace_bytes_smooth_jvp_ex") == args("dpr_workspace_bytes_jvp_ex")
        assert (getattr(L, f"dpr_raster_smooth_jvp_ex_{suf}").argtypes
                == getattr(L, f"dpr_raster_jvp_ex_{suf}").argtypes)
    for name in ("raster_smooth_jvp", "raster_smooth_jvp_", "resolve_algo_smooth_jvp", "workspace_bytes_smooth_jvp"):
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_is_the_tiled_smooth_forwards(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_smooth_jvp_ex_{suf}")
    fwd = getattr(L, f"dpr_workspace_bytes_smooth_ex_{suf}")
    for n_in, n_out in PAIRS:
        a, gp = _g(GRIDS[n_out])
        for K in (1, 16):
            for B in (1, 7):
                assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, B, K) == 0
                for P in (1, 1000, 1_000_000):
                    want = fwd(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, B)
                    assert want not in (0, SIZE_MAX)
                    assert f(_lib.ALGO_TILED, 0, n_in, n_out, gp, P, B, K) == want
                    for fl in (_lib.FLAG_NO_POINT_WEIGHT_GRAD, _lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4)):
                        assert f(_lib.ALGO_TILED, fl, n_in, n_out, gp, P, B, K) == want
                assert f(_lib.ALGO_TILED, 0, n_in, n_out, gp, 0, B, K) == 0
                assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, 0, B, K) == 0
        # AUTO's workspace is that of the algorithm it resolves to
        for P in (1000, 10**6):
            auto = L.dpr_resolve_algo_smooth_jvp(n_in, n_out, gp, P, 2, 3)
            assert f(_lib.ALGO_AUTO, 0, n_in, n_out, gp, P, 2, 3) == f(auto, 0, n_in, n_out, gp, P, 2, 3)
        # the refused combinations
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            assert f(algo, 0, n_in, n_out, gp, 1000, 3, 2) == SIZE_MAX
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            assert f(_lib.ALGO_AUTO, fl, n_in, n_out, gp, 1000, 3, 2) == SIZE_MAX
        for K in (0, 17, -1):
            assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, K) == SIZE_MAX
        assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, -1, 3, 2) == SIZE_MAX
        assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, -1, 2) == SIZE_MAX
        assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, None, 10, 1, 2) == SIZE_MAX
        assert f(_lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 1) == SIZE_MAX  # smooth_tile_count == 0
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            assert f(_lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 1) == SIZE_MAX, (n_in, n_out)
    # the Python mirror
    assert dpr_amd.workspace_bytes_smooth_jvp((16, 16), 10, 2, 3, 4, algo="atomic") == 0
    assert (dpr_amd.workspace_bytes_smooth_jvp((16, 16), 10, 2, 3, 4, algo="tiled")
            == dpr_amd.workspace_bytes_smooth("raster", (16, 16), 10, 2, 3, algo="tiled"))
    for kw in (dict(algo="chunked"), dict(algo="ordered"), dict(tangents=17)):
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.workspace_bytes_smooth_jvp((16, 16, 16), 10, 2, 3, **kw)


def test_resolve_algo_smooth_jvp_matches_the_recorded_table():
    """AUTO on the probe's rows (tests/golden/smooth_jvp_auto.json, written by tools/smooth_jvp_probe.py: shape, K,
    the two measured times, AUTO's choice): the choice is still AUTO's, and it is within 1.15x of the faster path --
    the margin tests/test_smooth_abi.py holds the smooth forward to."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_jvp_auto.json")))
    L = dpr_amd.lib()
    assert len(table["shapes"]) >= 18  # six shapes, K = 1, 4, 12
    for row in table["shapes"]:
        a, gp = _g(row["grid"])
        got = L.dpr_resolve_algo_smooth_jvp(row["n_in"], len(row["grid"]), gp, row["P"], row["B"], row["K"])
        assert got == _lib.ALGOS[row["auto"]], row
        assert dpr_amd.resolve_algo_smooth_jvp(row["grid"], row["P"], row["B"], row["n_in"], row["K"]) == row["auto"]
        t = row["ms"]
        assert t[row["auto"]] <= 1.15 * min(t.values()), row
    # The rule the table decided (csrc/dpr_api_smooth.hip): TILED from P * K = 1e5 on a 3-D grid and 4e5 on a 2-D grid,
    # where the tiled path can run the call; whatever B; never another algorithm.  For K = 1 on a 3-D grid that is
    # the smooth forward's rule for one pose.
    for n_in, n_out in PAIRS:
        work = 100_000 if n_out == 3 else 400_000
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 6249, 6250, 24_999, 25_000, 99_999, 10**5, 399_999, 4 * 10**5, 10**6, 10**7, 10**9,
                      (1 << 32) - 2, (1 << 32) - 1):
                for B in (1, 16, 1000):
                    for K in (1, 4, 16):
                        got = L.dpr_resolve_algo_smooth_jvp(n_in, n_out, gp, P, B, K)
                        can = L.dpr_workspace_bytes_smooth_ex_f32(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp,
                                                                  P, 1) != SIZE_MAX
                        want = _lib.ALGO_TILED if P * K >= work and can else _lib.ALGO_ATOMIC
                        assert got == want, (grid, P, B, K)
                        if K == 1 and n_out == 3:
                            assert got == L.dpr_resolve_algo_smooth(_lib.OP_RASTER, n_in, n_out, gp, P, 1)
    a, gp = _g((64, 64))
    assert L.dpr_resolve_algo_smooth_jvp(3, 2, gp, 100, 2, 0) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_smooth_jvp(3, 2, gp, 100, 2, 17) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_smooth_jvp(0, 2, gp, 100, 2, 1) == _lib.ERR_UNSUPPORTED_DIMS
    assert L.dpr_resolve_algo_smooth_jvp(2, 3, gp, 100, 2, 1) == _lib.ERR_UNSUPPORTED_DIMS
    assert L.dpr_resolve_algo_smooth_jvp(3, 2, None, 100, 2, 1) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_smooth_jvp(3, 2, gp, -1, 2, 1) == _lib.ERR_INVALID_ARG


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    a0, gp0 = _g((16, 0, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fn = getattr(L, f"dpr_raster_smooth_jvp_ex_{suf}")

        def f(algo=_lib.ALGO_ATOMIC, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, out=d, pts=d, rot=d, trans=d, grid=gp,
              tans=(d, d, d, d, d, d), ws=None, wsb=0):
            return fn(None, algo, flags, n_in, n_out, grid, P, B, K, out, pts, rot, trans, None, None, *tans, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        for n_in, n_out in ALL_PAIRS:
            if (n_in, n_out) not in PAIRS:
                refused(f(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        refused(f(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        for K in (0, 17, -3):
            refused(f(K=K), _lib.ERR_INVALID_ARG, "tangents K")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        refused(f(grid=gp0), _lib.ERR_INVALID_ARG, "out of range")
        refused(f(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(P=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(out=None), _lib.ERR_INVALID_ARG, "out_dot is NULL")
        refused(f(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(f(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(out=odd), _lib.ERR_INVALID_ARG, "aligned")
        for k in range(6):
            refused(f(tans=tuple(odd if i == k else d for i in range(6))), _lib.ERR_INVALID_ARG, "aligned")
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            refused(f(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            refused(f(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(f(algo=_lib.ALGO_TILED, P=(1 << 32) - 1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")
        # the tiled path: no workspace, one too small, one misaligned
        need = getattr(L, f"dpr_workspace_bytes_smooth_jvp_ex_{suf}")(_lib.ALGO_TILED, 0, 3, 3, gp, 10, 2, 3)
        assert need not in (0, SIZE_MAX)
        refused(f(algo=_lib.ALGO_TILED), _lib.ERR_WORKSPACE, "workspace")
        refused(f(algo=_lib.ALGO_TILED, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
        refused(f(algo=_lib.ALGO_TILED, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        # B = 0: nothing to write, after the checks
        assert f(B=0) == _lib.OK
        refused(f(B=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "DPR_ALGO_ATOMIC and DPR_ALGO_TILED")
        refused(f(B=0, K=17), _lib.ERR_INVALID_ARG, "tangents K")


def test_python_wrappers_raise_without_a_device():
    pts = torch.zeros(10, 3)
    R, t = torch.zeros(4, 2, 3), torch.zeros(4, 2)
    bad = [
        dict(points=torch.zeros(4, 10, 3)),                  # not (P, N_in)
        dict(points=torch.zeros(10, 2)),                     # N_in differs from rotation's columns
        dict(translation=torch.zeros(3, 2)),                 # B differs
        dict(rotation=torch.zeros(4, 3, 2), points=torch.zeros(10, 2), translation=torch.zeros(4, 3)),  # (2, 3)
        dict(rotation=torch.zeros(4, 4), points=torch.zeros(10, 4), translation=torch.zeros(4)),         # (4, 4)
    ]
    for kw in bad:
        a = dict(points=pts, rotation=R, translation=t)
        a.update(kw)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_jvp((16, 16), a["points"], a["rotation"], a["translation"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.raster_smooth_jvp_(torch.zeros(16, 16, 4), a["points"], a["rotation"], a["translation"])
    for K in (0, 17, True, 2.0):
        with pytest.raises(dpr_amd.DprError):
            dpr_amd.raster_smooth_jvp((16, 16), pts, R, t, tangents=K)
    # consistent shapes on the CPU: there is no CPU path
    with pytest.raises(RuntimeError):
        dpr_amd.raster_smooth_jvp((16, 16), pts, R, t, points_dot=torch.zeros(10, 3))
    # libdpr's own refusals come back as DprError
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_jvp((16, 16, 16), 10, 4, 2)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_smooth_jvp((16, 16), 10, 4, 3, 17)
