"""Host-side checks of the multi-channel C ABI (include/dpr.h, MULTI-CHANNEL): prototypes and exports,
workspace sizes, the AUTO rule and argument errors.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpr_amd
from dpr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_raster_channels_ex_f32", "dpr_raster_channels_ex_f64",
       "dpr_raster_pullback_channels_ex_f32", "dpr_raster_pullback_channels_ex_f64",
       "dpr_workspace_bytes_channels_ex_f32", "dpr_workspace_bytes_channels_ex_f64",
       "dpr_resolve_algo_channels"]
SIZE_MAX = ctypes.c_size_t(-1).value
C3 = (256, 256, 256)


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_channel_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert L.dpr_version() >= 106


@pytest.mark.parametrize("suf,elem", [("f32", 4), ("f64", 8)])
def test_workspace_bytes_channels(suf, elem):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_channels_ex_{suf}")
    a, gp = _g(C3)
    P = 10_000_000
    for C in (0, 17):
        assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp, P, 1, C) == SIZE_MAX
        assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 3, gp, P, 1, C) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 5, 3, gp, P, 1, 3) == SIZE_MAX  # n_in = 5
    single = getattr(L, f"dpr_workspace_bytes_ex_{suf}")(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp, P, 1)
    assert single != SIZE_MAX and single > 0
    for C in (1, 3, 16):
        n = f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp, P, 1, C)
        assert n != SIZE_MAX and n >= single + C * P * elem
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 3, gp, P, 1, 3) == 0
    assert f(_lib.OP_PULLBACK, _lib.ALGO_ATOMIC, 0, 3, 3, gp, P, 1, 3) == 0
    # refused: chunked, a tiled pullback, sharing flags, the residual op, tiled on a direct-only pair
    assert f(_lib.OP_RASTER, _lib.ALGO_CHUNKED, 0, 3, 3, gp, P, 1, 3) == SIZE_MAX
    assert f(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, 3, 3, gp, P, 1, 3) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_TILED, _lib.FLAG_KEEP_BINNING, 3, 3, gp, P, 1, 3) == SIZE_MAX
    assert f(_lib.OP_PULLBACK, _lib.ALGO_AUTO, _lib.FLAG_REUSE_BINNING, 3, 3, gp, P, 1, 3) == SIZE_MAX
    assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_AUTO, 0, 3, 3, gp, P, 1, 3) == SIZE_MAX
    a2, gp2 = _g((64, 64, 64))
    assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 2, 3, gp2, P, 1, 3) == SIZE_MAX


def test_resolve_algo_channels():
    L = dpr_amd.lib()
    a, gp = _g(C3)
    P = 10_000_000
    assert L.dpr_resolve_algo_channels(_lib.OP_RASTER, 3, 3, gp, P, 1, 3) == _lib.ALGO_TILED
    for C in (1, 3, 16):
        assert L.dpr_resolve_algo_channels(_lib.OP_PULLBACK, 3, 3, gp, P, 1, C) == _lib.ALGO_ATOMIC
    a3, gp3 = _g((64, 64, 64))
    assert L.dpr_resolve_algo_channels(_lib.OP_RASTER, 2, 3, gp3, P, 1, 3) == _lib.ALGO_ATOMIC
    shapes = [(C3, 3, 3, P, 1), (C3, 3, 3, 1000, 1), ((128,) * 3, 3, 3, 1_000_000, 1),
              ((512, 512), 3, 2, P, 8), ((512, 512), 2, 2, 10_000, 4), ((64,) * 4, 4, 4, 10_000, 1)]
    for grid, n_in, n_out, p, b in shapes:
        ag, gg = _g(grid)
        for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
            r1 = L.dpr_resolve_algo_channels(op, n_in, n_out, gg, p, b, 1)
            assert r1 in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)
            assert L.dpr_resolve_algo_channels(op, n_in, n_out, gg, p, b, 16) == r1, (grid, op)
    assert L.dpr_resolve_algo_channels(_lib.OP_RASTER, 3, 3, gp, P, 1, 0) == _lib.ERR_INVALID_ARG
    assert L.dpr_resolve_algo_channels(_lib.OP_RASTER, 3, 3, gp, P, 1, 17) == _lib.ERR_INVALID_ARG
    assert "C = 17" in _lib.last_error()
    # the Python mirror
    assert dpr_amd.resolve_algo_channels("raster", C3, P, 1, 3, 3) == "tiled"
    assert dpr_amd.resolve_algo_channels("pullback", C3, P, 1, 3, 3) == "atomic"


def test_channel_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument errors come back as statuses from the host checks (NULL device pointers: nothing could
    run, and nothing is launched -- no GPU is touched)."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    rot = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the host checks
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_raster_channels_ex_{suf}")
        bwd = getattr(L, f"dpr_raster_pullback_channels_ex_{suf}")
        for C in (0, 17):
            assert fwd(None, 0, 0, 3, 3, gp, 10, 1, C, rot, rot, rot, rot, None, None, None, None, 0) \
                == _lib.ERR_INVALID_ARG
            assert bwd(None, 0, 0, 3, 3, gp, 10, 1, C, rot, rot, rot, rot, None, None,
                       rot, rot, rot, rot, rot, rot, None, 0) == _lib.ERR_INVALID_ARG
        assert fwd(None, _lib.ALGO_CHUNKED, 0, 3, 3, gp, 10, 1, 3, rot, rot, rot, rot, None, None, None, None,
                   0) == _lib.ERR_UNSUPPORTED_ALGO
        assert fwd(None, _lib.ALGO_TILED, _lib.FLAG_KEEP_BINNING, 3, 3, gp, 10, 1, 3, rot, rot, rot, rot,
                   None, None, None, None, 0) == _lib.ERR_UNSUPPORTED_ALGO
        assert fwd(None, _lib.ALGO_TILED, 0, 2, 3, gp, 10, 1, 3, rot, rot, rot, rot, None, None, None, None,
                   0) == _lib.ERR_UNSUPPORTED_ALGO
        assert bwd(None, _lib.ALGO_TILED, 0, 3, 3, gp, 10, 1, 3, rot, rot, rot, rot, None, None,
                   rot, rot, rot, rot, rot, rot, None, 0) == _lib.ERR_UNSUPPORTED_ALGO
        assert fwd(None, 0, 0, 5, 3, gp, 10, 1, 3, rot, rot, rot, rot, None, None, None, None, 0) \
            == _lib.ERR_UNSUPPORTED_DIMS
        assert fwd(None, 0, 0, 3, 3, gp, 10, 1, 3, None, rot, rot, rot, None, None, None, None, 0) \
            == _lib.ERR_INVALID_ARG  # out is NULL
