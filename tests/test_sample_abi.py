"""Host-side checks of the sampling C ABI (include/dpr.h, SAMPLING): prototypes and exports, workspace sizes,
the AUTO rule and argument errors.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpr_amd
from dpr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_sample_ex_f32", "dpr_sample_ex_f64", "dpr_sample_pullback_ex_f32", "dpr_sample_pullback_ex_f64",
       "dpr_workspace_bytes_sample_ex_f32", "dpr_workspace_bytes_sample_ex_f64", "dpr_resolve_algo_sample"]
SIZE_MAX = ctypes.c_size_t(-1).value
C3 = (256, 256, 256)
PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_sampling_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert L.dpr_version() >= 107
    for name in ("sample", "sample_", "sample_pullback_", "sample_ad", "resolve_algo_sample",
                 "workspace_bytes_sample"):
        assert callable(getattr(dpr_amd, name)), name


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes_sample(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_sample_ex_{suf}")
    single = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    a, gp = _g(C3)
    P = 10_000_000
    for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
        for n_in, n_out in PAIRS:
            ag, gg = _g((16,) * n_out)
            assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gg, 1000, 3) == 0, (op, n_in, n_out)
    assert f(_lib.OP_RASTER, _lib.ALGO_AUTO, 0, 3, 3, gp, P, 4) == 0
    # the tiled pullback: at least the single-channel tiled forward workspace of (grid, P, B = 1), for any B
    for grid, n_in in ((C3, 3), ((512, 512), 3), ((512, 512), 2), ((128,) * 3, 3)):
        ag, gg = _g(grid)
        ref = single(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, len(grid), gg, P, 1)
        assert ref not in (0, SIZE_MAX)
        for B in (1, 8):
            n = f(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, n_in, len(grid), gg, P, B)
            assert n != SIZE_MAX and n >= ref, (grid, B)
    # refused: bad dims, a bad op, the tiled / chunked forward, chunked pullback, tiled on a direct-only
    # pair, the sharing flags
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 5, 3, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_ATOMIC, 0, 3, 0, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_AUTO, 0, 3, 3, gp, P, 1) == SIZE_MAX
    assert f(7, _lib.ALGO_AUTO, 0, 3, 3, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_TILED, 0, 3, 3, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_RASTER, _lib.ALGO_CHUNKED, 0, 3, 3, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_PULLBACK, _lib.ALGO_CHUNKED, 0, 3, 3, gp, P, 1) == SIZE_MAX
    a2, gp2 = _g((64, 64, 64))
    assert f(_lib.OP_PULLBACK, _lib.ALGO_TILED, 0, 2, 3, gp2, P, 1) == SIZE_MAX
    assert f(_lib.OP_PULLBACK, _lib.ALGO_AUTO, _lib.FLAG_KEEP_BINNING, 3, 3, gp, P, 1) == SIZE_MAX
    assert f(_lib.OP_PULLBACK, _lib.ALGO_AUTO, _lib.FLAG_REUSE_BINNING, 3, 3, gp, P, 1) == SIZE_MAX
    # the Python mirror
    assert dpr_amd.workspace_bytes_sample("sample", C3, P, 1, 3) == 0
    assert dpr_amd.workspace_bytes_sample("pullback", C3, P, 1, 3, algo="tiled") >= \
        dpr_amd.workspace_bytes("raster", C3, P, 1, 3, algo="tiled")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes_sample("sample", C3, P, 1, 3, algo="tiled")


def test_resolve_algo_sample():
    L = dpr_amd.lib()
    shapes = [(C3, 3, 3, 10_000_000, 1), (C3, 3, 3, 1000, 1), ((128,) * 3, 3, 3, 1_000_000, 1),
              ((512, 512), 3, 2, 10_000_000, 8), ((512, 512), 2, 2, 10_000, 4), ((64,) * 4, 4, 4, 10_000, 1),
              ((64, 64, 64), 2, 3, 10_000_000, 2)]
    for grid, n_in, n_out, P, B in shapes:
        ag, gg = _g(grid)
        # the forward: always the direct gather
        assert L.dpr_resolve_algo_sample(_lib.OP_RASTER, n_in, n_out, gg, P, B) == _lib.ALGO_ATOMIC
        # the pullback: tiled where the single-pose forward of the shape is
        fwd1 = L.dpr_resolve_algo(_lib.OP_RASTER, n_in, n_out, gg, P, 1)
        want = _lib.ALGO_TILED if fwd1 == _lib.ALGO_TILED else _lib.ALGO_ATOMIC
        assert L.dpr_resolve_algo_sample(_lib.OP_PULLBACK, n_in, n_out, gg, P, B) == want, (grid, P, B)
    a, gp = _g(C3)
    assert L.dpr_resolve_algo_sample(_lib.OP_PULLBACK, 3, 3, gp, 10_000_000, 1) == _lib.ALGO_TILED
    assert L.dpr_resolve_algo_sample(_lib.OP_PULLBACK, 3, 3, gp, 1000, 1) == _lib.ALGO_ATOMIC
    assert L.dpr_resolve_algo_sample(_lib.OP_RASTER, 5, 3, gp, 1000, 1) == _lib.ERR_UNSUPPORTED_DIMS
    assert L.dpr_resolve_algo_sample(_lib.OP_RESIDUAL_PULLBACK, 3, 3, gp, 1000, 1) == _lib.ERR_INVALID_ARG
    assert "op 2" in _lib.last_error()
    assert dpr_amd.resolve_algo_sample("sample", C3, 10_000_000, 1, 3) == "atomic"
    assert dpr_amd.resolve_algo_sample("pullback", C3, 10_000_000, 1, 3) == "tiled"


def test_sampling_entry_points_refuse_bad_arguments_before_any_launch():
    """Argument errors come back as statuses from the host checks (dummy device pointers that are never
    dereferenced: every call below fails before anything is launched -- no GPU is touched)."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    d = ctypes.c_void_p(256)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_sample_ex_{suf}")
        bwd = getattr(L, f"dpr_sample_pullback_ex_{suf}")

        def f(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, values=d, image=d, pts=d, rot=d, trans=d, ws=None,
              wsb=0):
            return fwd(None, algo, flags, n_in, n_out, gp, P, B, values, image, pts, rot, trans, ws, wsb)

        def b(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, dv=d, image=d, pts=d, rot=d, trans=d,
              outs=(d, d, d, d), ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, gp, P, B, dv, image, pts, rot, trans, *outs, ws, wsb)

        assert f(n_in=5) == _lib.ERR_UNSUPPORTED_DIMS
        assert f(n_out=0) == _lib.ERR_UNSUPPORTED_DIMS
        assert f(algo=_lib.ALGO_TILED) == _lib.ERR_UNSUPPORTED_ALGO
        assert "ATOMIC only" in _lib.last_error()
        assert f(algo=_lib.ALGO_CHUNKED) == _lib.ERR_UNSUPPORTED_ALGO
        assert f(flags=_lib.FLAG_KEEP_BINNING) == _lib.ERR_UNSUPPORTED_ALGO
        assert f(values=None) == _lib.ERR_INVALID_ARG
        assert "values" in _lib.last_error()
        assert f(image=None) == _lib.ERR_INVALID_ARG
        assert f(pts=None) == _lib.ERR_INVALID_ARG
        assert f(rot=None) == _lib.ERR_INVALID_ARG
        assert f(trans=None) == _lib.ERR_INVALID_ARG
        assert f(P=-1) == _lib.ERR_INVALID_ARG
        assert f(values=ctypes.c_void_p(258)) == _lib.ERR_INVALID_ARG  # misaligned
        # (nothing to do: no launch, success)
        assert f(P=0, values=None, image=None, pts=None) == _lib.OK
        assert f(B=0, values=None, image=None) == _lib.OK

        assert b(n_in=5) == _lib.ERR_UNSUPPORTED_DIMS
        assert b(outs=(None, None, None, None)) == _lib.ERR_INVALID_ARG
        assert "every output is NULL" in _lib.last_error()
        assert b(algo=_lib.ALGO_CHUNKED) == _lib.ERR_UNSUPPORTED_ALGO
        assert b(n_in=2, algo=_lib.ALGO_TILED) == _lib.ERR_UNSUPPORTED_ALGO
        assert b(flags=_lib.FLAG_REUSE_BINNING) == _lib.ERR_UNSUPPORTED_ALGO
        assert b(dv=None) == _lib.ERR_INVALID_ARG
        assert b(pts=None) == _lib.ERR_INVALID_ARG
        assert b(rot=None) == _lib.ERR_INVALID_ARG
        assert b(image=None) == _lib.ERR_INVALID_ARG  # ds_dpoints etc. read the image
        assert b(outs=(d, None, d, None), dv=ctypes.c_void_p(262)) == _lib.ERR_INVALID_ARG  # misaligned
        # the tiled pullback's ds_dimage needs the workspace of the single-pose tiled forward
        assert b(algo=_lib.ALGO_TILED) == _lib.ERR_WORKSPACE
        assert b(algo=_lib.ALGO_TILED, ws=d, wsb=16) == _lib.ERR_WORKSPACE
        assert b(algo=_lib.ALGO_TILED, ws=ctypes.c_void_p(300), wsb=1 << 40) == _lib.ERR_WORKSPACE  # misaligned


def test_python_api_refuses_cpu_tensors_and_bad_need():
    import torch

    pts = torch.zeros((4, 3))
    img = torch.zeros((8, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.sample(img, pts, torch.eye(3), torch.zeros(3))
    with pytest.raises(ValueError, match="unknown gradient"):
        dpr_amd.sample_pullback_(torch.zeros(4), img, pts, torch.eye(3), torch.zeros(3), need=("weights",))
    with pytest.raises(ValueError, match="at least one"):
        dpr_amd.sample_pullback_(torch.zeros(4), img, pts, torch.eye(3), torch.zeros(3), need=())
