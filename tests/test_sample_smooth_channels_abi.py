"""Host-side checks of the C ABI of smooth sampling of C-channel images (include/dpr.h, SMOOTH SAMPLING,
MULTI-CHANNEL): prototypes and exports, the AUTO rule against dpr_resolve_algo_smooth_channels, workspace sizes, every
refusal.  No GPU needed: every refused call returns before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpr_amd
from dpr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_resolve_algo_sample_smooth_channels", "dpr_workspace_bytes_sample_smooth_channels_ex_f32",
       "dpr_workspace_bytes_sample_smooth_channels_ex_f64", "dpr_sample_smooth_channels_ex_f32",
       "dpr_sample_smooth_channels_ex_f64", "dpr_sample_smooth_channels_pullback_ex_f32",
       "dpr_sample_smooth_channels_pullback_ex_f64"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
RASTER, PULLBACK = _lib.OP_RASTER, _lib.OP_PULLBACK


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)
    L = dpr_amd.lib()
    assert len(NEW) == 7
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in ("sample_smooth_channels", "sample_smooth_channels_", "sample_smooth_channels_pullback_",
                 "sample_smooth_channels_ad", "resolve_algo_sample_smooth_channels"):
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    # no public workspace query for this family: every call asks and allocates (tests/workspace_cases.py lists the
    # public ones)
    assert not hasattr(dpr_amd, "workspace_bytes_sample_smooth_channels")
    assert "SMOOTH SAMPLING, MULTI-CHANNEL" in open(os.path.join(ROOT, "include", "dpr.h")).read()


def test_prototypes_follow_dpr_sample_smooth_with_c_after_b():
    text = open(os.path.join(ROOT, "include", "dpr.h")).read()

    def proto(name):
        m = re.search(rf"\b{name}\s*\((.*?)\);", text, flags=re.S)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1))

    for suffix in ("", "_ex_f32", "_ex_f64"):
        head = "dpr_resolve_algo_sample_smooth" if not suffix else "dpr_workspace_bytes_sample_smooth"
        new = proto(head + "_channels" + suffix)
        assert new == proto(head + suffix) + ", int64_t C", new
    for name in ("dpr_sample_smooth{}_ex_f32", "dpr_sample_smooth{}_ex_f64", "dpr_sample_smooth{}_pullback_ex_f32",
                 "dpr_sample_smooth{}_pullback_ex_f64"):
        assert proto(name.format("_channels")) == proto(name.format("")).replace("int64_t B,", "int64_t B, int64_t C,")


def test_auto_is_atomic_forward_and_the_smooth_channel_forwards_choice_for_the_pullback():
    """Shapes on both sides of the constants of dpr_resolve_algo_smooth_channels (3-D: P * C >= 1e5, 2-D: P * C >=
    3e5, and a grid whose tiles fit the sort key)."""
    L = dpr_amd.lib()
    seen = set()
    for n_in, n_out in PAIRS:
        grids = [(8,) * n_out, (37, 19, 21) if n_out == 3 else (150, 37), (128,) * n_out,
                 (32768,) * 2 if n_out == 2 else (1290,) * 3]
        for grid in grids:
            a, gp = _g(grid)
            for P in (0, 1, 6_249, 6_250, 18_749, 18_750, 33_333, 33_334, 99_999, 100_000, 299_999, 300_000, 10**6,
                      (1 << 32) - 2, (1 << 32) - 1):
                for C in (1, 3, 4, 16):
                    for B in (1, 3, 64):
                        assert L.dpr_resolve_algo_sample_smooth_channels(RASTER, n_in, n_out, gp, P, B,
                                                                         C) == _lib.ALGO_ATOMIC
                        want = L.dpr_resolve_algo_smooth_channels(RASTER, n_in, n_out, gp, P, 1, C)
                        assert want in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)
                        got = L.dpr_resolve_algo_sample_smooth_channels(PULLBACK, n_in, n_out, gp, P, B, C)
                        assert got == want, (grid, P, B, C)
                        seen.add((n_out, got))
                        if got == _lib.ALGO_TILED:  # only where the tiled path can run
                            assert L.dpr_workspace_bytes_sample_smooth_channels_ex_f32(PULLBACK, 0, 0, n_in, n_out, gp,
                                                                                       P, B, C) != SIZE_MAX
    assert seen == {(n, a) for n in (2, 3) for a in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)}
    # the thresholds themselves, and the Python mirror
    r = dpr_amd.resolve_algo_sample_smooth_channels
    assert r("pullback", (64, 64, 64), 6_249, 4, 3, 16) == "atomic"
    assert r("pullback", (64, 64, 64), 6_250, 4, 3, 16) == "tiled"
    assert r("pullback", (64, 64), 99_999, 4, 3, 3) == "atomic"
    assert r("pullback", (64, 64), 100_000, 4, 2, 3) == "tiled"
    assert r("sample", (64, 64), 100_000, 4, 2, 3) == "atomic"
    assert r("raster", (64, 64, 64), 10**6, 4, 3, 16) == "atomic"
    a, gp = _g((64, 64))
    f = L.dpr_resolve_algo_sample_smooth_channels
    assert f(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2, 3) == _lib.ERR_INVALID_ARG
    assert f(RASTER, 2, 3, gp, 100, 2, 3) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(RASTER, 3, 2, None, 100, 2, 3) == _lib.ERR_INVALID_ARG
    assert f(RASTER, 3, 2, gp, -1, 2, 3) == _lib.ERR_INVALID_ARG
    for C in (0, 17, -1):
        assert f(PULLBACK, 3, 2, gp, 100, 2, C) == _lib.ERR_INVALID_ARG
        assert "channels C" in _lib.last_error()
    with pytest.raises(dpr_amd.DprError):
        r("sample", (16, 16, 16), 10, 4, 2, 3)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_bytes(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_sample_smooth_channels_ex_{suf}")
    smooth = getattr(L, f"dpr_workspace_bytes_smooth_ex_{suf}")
    for n_in, n_out in PAIRS:
        a, gp = _g((37, 19, 21) if n_out == 3 else (150, 37))
        for C in (1, 3, 16):
            for op in (RASTER, PULLBACK):
                for B in (1, 4, 64):
                    assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, B, C) == 0
                    assert f(op, _lib.ALGO_ATOMIC, _lib.FLAG_COHERENT_POINTS, n_in, n_out, gp, 1000, B, C) == 0
                assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, C) == 0
            # the TILED pullback: the workspace of the tiled smooth forward of one pose, whatever B and C
            for P in (1, 1000, 20_000, 1_000_000):
                want = smooth(RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, 1)
                assert want not in (0, SIZE_MAX)
                for B in (1, 4, 64):
                    assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, P, B, C) == want
            assert f(PULLBACK, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1_000_000, 4, C) == \
                smooth(RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1_000_000, 1)
            assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, 0, 4, C) == 0
        # the refused combinations
        assert f(RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1000, 3, 3) == SIZE_MAX
        assert "forward runs on DPR_ALGO_ATOMIC only" in _lib.last_error()
        for op in (RASTER, PULLBACK):
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, 3) == SIZE_MAX
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC, _lib.ALGO_TILED):
                    assert f(op, algo, fl, n_in, n_out, gp, 1000, 3, 3) == SIZE_MAX
            for C in (0, 17, -3):
                for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC, _lib.ALGO_TILED):
                    assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, C) == SIZE_MAX
        assert f(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 3) == SIZE_MAX
        assert f(RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, -1, 3, 3) == SIZE_MAX
        assert f(RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, -1, 3) == SIZE_MAX
        assert f(RASTER, _lib.ALGO_ATOMIC, 0, n_in, n_out, None, 10, 1, 3) == SIZE_MAX
        # the limits of the tiled smooth forward
        assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 3) == SIZE_MAX
        assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 2, 1, 3) != SIZE_MAX
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            for op in (RASTER, PULLBACK):
                assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 3) == SIZE_MAX, (n_in, n_out)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy device pointers that are never dereferenced: every call below fails in the host checks."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_sample_smooth_channels_ex_{suf}")
        bwd = getattr(L, f"dpr_sample_smooth_channels_pullback_ex_{suf}")

        def f(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, C=3, values=d, image=d, pts=d, rot=d, trans=d, grid=gp,
              ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, C, values, image, pts, rot, trans, ws, wsb)

        def b(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, C=3, dv=d, image=d, pts=d, rot=d, trans=d,
              outs=(d, d, d, d), ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, gp, P, B, C, dv, image, pts, rot, trans, *outs, ws, wsb)

        def refused(rc, code, text):
            assert rc == code, (rc, code, _lib.last_error())
            assert text in _lib.last_error(), _lib.last_error()

        for n_in, n_out in ALL_PAIRS:
            if (n_in, n_out) not in PAIRS:
                refused(f(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
                refused(b(n_in=n_in, n_out=n_out), _lib.ERR_UNSUPPORTED_DIMS, "supports (2,2), (3,3), (3,2)")
        refused(f(n_in=5), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        refused(b(n_out=0), _lib.ERR_UNSUPPORTED_DIMS, "unsupported")
        for C in (0, 17, -1):
            refused(f(C=C), _lib.ERR_INVALID_ARG, "channels C")
            refused(b(C=C), _lib.ERR_INVALID_ARG, "channels C")
        refused(f(algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "forward runs on DPR_ALGO_ATOMIC only")
        for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
            refused(f(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "not algorithm")
            refused(b(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "not algorithm")
        for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
            refused(f(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            refused(b(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
        for op_flags in (_lib.FLAG_COHERENT_POINTS, _lib.FLAG_NO_POINT_WEIGHT_GRAD):  # accepted and ignored
            refused(f(flags=op_flags, values=None), _lib.ERR_INVALID_ARG, "values is NULL")
        refused(f(values=None), _lib.ERR_INVALID_ARG, "values is NULL")
        refused(f(image=None), _lib.ERR_INVALID_ARG, "image is NULL")
        refused(f(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(f(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(trans=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(f(grid=None), _lib.ERR_INVALID_ARG, "grid is NULL")
        refused(f(P=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(B=-1), _lib.ERR_INVALID_ARG, "negative")
        refused(f(values=odd), _lib.ERR_INVALID_ARG, "aligned")
        # (nothing to do: no launch, success)
        assert f(P=0, values=None, image=None, pts=None) == _lib.OK
        assert f(B=0, values=None, image=None) == _lib.OK
        refused(f(B=0, algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "ATOMIC only")
        refused(f(P=0, C=17), _lib.ERR_INVALID_ARG, "channels C")

        refused(b(outs=(None, None, None, None)), _lib.ERR_INVALID_ARG, "every output is NULL")
        refused(b(dv=None), _lib.ERR_INVALID_ARG, "ds_dvalues is NULL")
        refused(b(pts=None), _lib.ERR_INVALID_ARG, "points is NULL")
        refused(b(rot=None), _lib.ERR_INVALID_ARG, "rotation/translation")
        refused(b(image=None), _lib.ERR_INVALID_ARG, "image is NULL")  # ds_dpoints etc. read the image
        refused(b(image=None, outs=(d, None, d, None)), _lib.ERR_INVALID_ARG, "image is NULL")
        refused(b(outs=(d, None, d, None), dv=ctypes.c_void_p(262)), _lib.ERR_INVALID_ARG, "aligned")
        refused(b(outs=(d, d, odd, d)), _lib.ERR_INVALID_ARG, "aligned")
        # the tiled pullback's ds_dimage: no workspace, one too small, one misaligned, P beyond the sort's index
        need = getattr(L, f"dpr_workspace_bytes_sample_smooth_channels_ex_{suf}")(PULLBACK, _lib.ALGO_TILED, 0, 3, 3, gp,
                                                                                  10, 2, 3)
        assert need not in (0, SIZE_MAX)
        refused(b(algo=_lib.ALGO_TILED), _lib.ERR_WORKSPACE, "workspace")
        refused(b(algo=_lib.ALGO_TILED, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
        refused(b(algo=_lib.ALGO_TILED, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        refused(b(algo=_lib.ALGO_ATOMIC, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        refused(b(algo=_lib.ALGO_TILED, P=(1 << 32) - 1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")


def test_python_wrappers_raise_without_a_device():
    pts = torch.zeros(10, 3)
    img = torch.zeros(8, 8, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.sample_smooth_channels(img, pts, torch.eye(3), torch.zeros(3))
    pb = dpr_amd.sample_smooth_channels_pullback_
    with pytest.raises(ValueError, match="unknown gradient"):
        pb(torch.zeros(10, 3), img, pts, torch.eye(3), torch.zeros(3), need=("weights",))
    with pytest.raises(ValueError, match="at least one"):
        pb(torch.zeros(10, 3), img, pts, torch.eye(3), torch.zeros(3), need=())
    with pytest.raises(ValueError, match="not in need"):
        pb(torch.zeros(10, 3), img, pts, torch.eye(3), torch.zeros(3), need=("image",), ds_dpoints=torch.zeros(10, 3))
    # the pairs the smooth kernels have, checked before anything else
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.sample_smooth_channels(img, torch.zeros(10, 2), torch.zeros(3, 2), torch.zeros(3))       # (2, 3)
    with pytest.raises(dpr_amd.DimensionMismatch):
        dpr_amd.sample_smooth_channels_ad(torch.zeros(8, 3), pts, torch.zeros(1, 3), torch.zeros(1))    # (3, 1)
