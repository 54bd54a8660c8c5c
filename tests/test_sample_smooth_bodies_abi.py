"""Host-side checks of the C ABI of smooth sampling at the points of rigid bodies (include/dpr.h, SMOOTH SAMPLING,
RIGID BODIES): prototypes and exports, the AUTO rule on the rows of tests/golden/smooth_bodies_auto.json, the workspace
query against that of the tiled smooth rigid-body forward, every refusal with its status, and the Python shape checks.
No GPU needed: every refused call returns before anything is launched or written (the data pointers are dummies)."""
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
NEW = ["dpr_resolve_algo_sample_smooth_bodies", "dpr_workspace_bytes_sample_smooth_bodies_ex_f32",
       "dpr_workspace_bytes_sample_smooth_bodies_ex_f64", "dpr_sample_smooth_bodies_ex_f32",
       "dpr_sample_smooth_bodies_ex_f64", "dpr_sample_smooth_bodies_pullback_ex_f32",
       "dpr_sample_smooth_bodies_pullback_ex_f64"]
PYTHON = ["sample_smooth_bodies", "sample_smooth_bodies_", "sample_smooth_bodies_pullback_", "sample_smooth_bodies_ad",
          "resolve_algo_sample_smooth_bodies"]
SIZE_MAX = ctypes.c_size_t(-1).value
ALL_PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
PAIRS = [(2, 2), (3, 3), (3, 2)]
RASTER, PULLBACK = _lib.OP_RASTER, _lib.OP_PULLBACK
MPG = _lib.flag_max_pose_group


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_header_declares_and_library_exports_the_seven_symbols():
    raw = open(os.path.join(ROOT, "include", "dpr.h")).read()
    assert "SMOOTH SAMPLING, RIGID BODIES" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = dpr_amd.lib()
    assert len(NEW) == 7
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in PYTHON:
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    assert L.dpr_version() == 110
    assert int(re.search(r"#define DPR_VERSION (\d+)", raw).group(1)) == 110
    # no public query: tests/test_workspace_contract_table.py holds that list to its own table
    assert not any("bodies" in n for n in dir(dpr_amd) if n.startswith("workspace_bytes"))
    assert "no public workspace query" in sys.modules[dpr_amd.sample_smooth_bodies.__module__].__doc__


def test_prototypes_are_those_of_smooth_sampling_with_body_and_K():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpr.h")).read(), flags=re.S)

    def proto(name):
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]

    for stem in ("dpr_resolve_algo_sample_smooth", "dpr_workspace_bytes_sample_smooth_ex_f32",
                 "dpr_workspace_bytes_sample_smooth_ex_f64", "dpr_sample_smooth_ex_f32", "dpr_sample_smooth_ex_f64",
                 "dpr_sample_smooth_pullback_ex_f32", "dpr_sample_smooth_pullback_ex_f64"):
        new = stem.replace("sample_smooth", "sample_smooth_bodies")
        assert new in NEW
        want = proto(stem)
        k = want.index("int64_t B")
        want.insert(k + 1, "int64_t K")
        pts = [i for i, a in enumerate(want) if a.endswith("*points")]
        if pts:
            want.insert(pts[0] + 1, "const void *body")
        assert proto(new) == want, new


def test_auto_is_atomic_forward_and_the_smooth_body_forwards_choice_for_the_pullback():
    """On the rows of tests/golden/smooth_bodies_auto.json, and on a sweep that reaches both answers."""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "smooth_bodies_auto.json")))
    L = dpr_amd.lib()
    f = L.dpr_resolve_algo_sample_smooth_bodies
    names = {_lib.ALGO_ATOMIC: "atomic", _lib.ALGO_TILED: "tiled"}
    seen = set()
    assert len(table["shapes"]) >= 24
    for row in table["shapes"]:
        a, gp = _g(row["grid"])
        n_out = len(row["grid"])
        shape = (row["n_in"], n_out, gp, row["P"], row["B"], row["K"])
        assert f(RASTER, *shape) == _lib.ALGO_ATOMIC, row
        got = f(PULLBACK, *shape)
        assert got == L.dpr_resolve_algo_smooth_bodies(RASTER, *shape), row
        assert names[got] == row["auto"], row
        assert dpr_amd.resolve_algo_sample_smooth_bodies("pullback", row["grid"], row["P"], row["B"], row["K"],
                                                         row["n_in"]) == row["auto"]
        assert dpr_amd.resolve_algo_sample_smooth_bodies("sample", row["grid"], row["P"], row["B"], row["K"],
                                                         row["n_in"]) == "atomic"
        seen.add(got)
    assert seen == {_lib.ALGO_ATOMIC, _lib.ALGO_TILED}
    for n_in, n_out in PAIRS:
        for grid in ((8,) * n_out, (128,) * n_out, (1000,) * n_out if n_out == 2 else (512, 512, 512)):
            a, gp = _g(grid)
            for P in (0, 1, 999, 10**4, 10**5, 10**6, 10**9, (1 << 32) - 1):
                for B, K in ((1, 1), (16, 7), (1000, 1000)):
                    assert f(RASTER, n_in, n_out, gp, P, B, K) == _lib.ALGO_ATOMIC
                    got = f(PULLBACK, n_in, n_out, gp, P, B, K)
                    assert got == L.dpr_resolve_algo_smooth_bodies(RASTER, n_in, n_out, gp, P, B, K), (grid, P, B, K)
                    if got == _lib.ALGO_TILED:  # only where the tiled path can run
                        assert L.dpr_workspace_bytes_sample_smooth_bodies_ex_f32(PULLBACK, 0, 0, n_in, n_out, gp, P, B,
                                                                                 K) not in (0, SIZE_MAX)
    a, gp = _g((64, 64))
    assert f(_lib.OP_RESIDUAL_PULLBACK, 3, 2, gp, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert f(9, 3, 2, gp, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert f(RASTER, 2, 3, gp, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS
    assert f(RASTER, 2, 3, None, 100, 2, 2) == _lib.ERR_UNSUPPORTED_DIMS  # (the grid is not looked at first)
    assert f(RASTER, 3, 2, None, 100, 2, 2) == _lib.ERR_INVALID_ARG
    assert f(RASTER, 3, 2, gp, 100, 2, 0) == _lib.ERR_INVALID_ARG
    assert f(RASTER, 3, 2, gp, -1, 2, 2) == _lib.ERR_INVALID_ARG
    with pytest.raises(KeyError):
        dpr_amd.resolve_algo_sample_smooth_bodies("residual_pullback", (64, 64), 100, 2, 2, 3)
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_sample_smooth_bodies("sample", (64, 64), 100, 2, 0, 3)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_workspace_query(suf):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_sample_smooth_bodies_ex_{suf}")
    splat = getattr(L, f"dpr_workspace_bytes_smooth_bodies_ex_{suf}")
    T = _lib.ALGO_TILED
    for n_in, n_out in PAIRS:
        a, gp = _g((37, 19, 21) if n_out == 3 else (150, 37))
        # the forward, ATOMIC and P = 0: no workspace
        for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC):
            for op in (RASTER, PULLBACK):
                for P, B, K in ((1000, 3, 4), (0, 3, 1), (1000, 0, 2), (0, 0, 1)):
                    assert f(op, algo, 0, n_in, n_out, gp, P, B, K) == 0, (op, algo, P, B, K)
                assert f(op, algo, _lib.FLAG_COHERENT_POINTS, n_in, n_out, gp, 1000, 3, 4) == 0
        assert f(PULLBACK, T, 0, n_in, n_out, gp, 0, 4, 3) == 0
        # the TILED pullback: the query of the tiled smooth rigid-body forward at groups of 1, 2 and the default
        for P, B in ((1, 1), (1000, 7), (20_000, 16), (1_000_000, 40)):
            for K in (1, 5, 1 << 20):
                for cap in (1, 2, 0):
                    need = f(PULLBACK, T, MPG(cap), n_in, n_out, gp, P, B, K)
                    assert need not in (0, SIZE_MAX) and need % 256 == 0
                    assert need == splat(RASTER, T, MPG(cap), n_in, n_out, gp, P, B, K), (P, B, K, cap)
        assert f(PULLBACK, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1_000_000, 4, 3) \
            == splat(RASTER, T, 0, n_in, n_out, gp, 1_000_000, 4, 3)
        # the refused combinations
        assert f(RASTER, T, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
        assert "forward runs on DPR_ALGO_ATOMIC only" in _lib.last_error()
        for op in (RASTER, PULLBACK):
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                assert f(op, algo, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC) + ((T,) if op == PULLBACK else ()):
                    assert f(op, algo, fl, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
                    assert "binning" in _lib.last_error()
            for K in (0, -1):
                assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 3, K) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1, 1 << 31) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1000, 1 << 16, 1 << 15) == SIZE_MAX  # B * K = 2^31
            assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, (1 << 16) - 1, 1 << 15) == 0
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, -1, 3, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 10, -1, 4) == SIZE_MAX
            assert f(op, _lib.ALGO_AUTO, 0, n_in, n_out, None, 10, 1, 4) == SIZE_MAX
        # DPR_FLAG_MAX_POSE_GROUP anywhere but the TILED pullback
        for op, algo in ((RASTER, _lib.ALGO_AUTO), (RASTER, _lib.ALGO_ATOMIC), (PULLBACK, _lib.ALGO_ATOMIC),
                         (PULLBACK, _lib.ALGO_AUTO)):  # (AUTO is ATOMIC at this shape)
            assert f(op, algo, MPG(2), n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            assert "DPR_FLAG_MAX_POSE_GROUP" in _lib.last_error()
        for op in (_lib.OP_RESIDUAL_PULLBACK, 7, -1):
            assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 1000, 3, 4) == SIZE_MAX
            assert "op" in _lib.last_error()
        # TILED where smooth_tile_count is 0: P beyond 2^32 - 2
        assert f(PULLBACK, T, 0, n_in, n_out, gp, (1 << 32) - 1, 1, 2) == SIZE_MAX
        assert f(PULLBACK, T, 0, n_in, n_out, gp, (1 << 32) - 2, 1, 2) != SIZE_MAX
    for n_in, n_out in ALL_PAIRS:
        if (n_in, n_out) not in PAIRS:
            a, gp = _g((16,) * n_out)
            for op in (RASTER, PULLBACK):
                assert f(op, _lib.ALGO_ATOMIC, 0, n_in, n_out, gp, 10, 1, 2) == SIZE_MAX, (n_in, n_out)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy aligned device pointers that are never dereferenced: every call below fails in the host checks, so no
    output is touched (a touched dummy would come back as DPR_ERR_HIP or a crash, not as the status asked for)."""
    L = dpr_amd.lib()
    a, gp = _g((16, 16, 16))
    bad_grid, bgp = _g((16, 0, 16))
    d = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"dpr_sample_smooth_bodies_ex_{suf}")
        bwd = getattr(L, f"dpr_sample_smooth_bodies_pullback_ex_{suf}")
        query = getattr(L, f"dpr_workspace_bytes_sample_smooth_bodies_ex_{suf}")

        def f(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, values=d, image=d, pts=d, body=d, rot=d, trans=d,
              grid=gp, ws=None, wsb=0):
            return fwd(None, algo, flags, n_in, n_out, grid, P, B, K, values, image, pts, body, rot, trans, ws, wsb)

        def b(algo=0, flags=0, n_in=3, n_out=3, P=10, B=2, K=3, dv=d, image=d, pts=d, body=d, rot=d, trans=d,
              outs=(d, d, d, d), grid=gp, ws=None, wsb=0):
            return bwd(None, algo, flags, n_in, n_out, grid, P, B, K, dv, image, pts, body, rot, trans, *outs, ws,
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
            refused(call(image=None), _lib.ERR_INVALID_ARG, "image is NULL")
            refused(call(pts=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(rot=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(body=odd), _lib.ERR_INVALID_ARG, "aligned")
            refused(call(ws=odd, wsb=1024), _lib.ERR_WORKSPACE, "256-byte aligned")
            # DPR_ERR_UNSUPPORTED_ALGO: CHUNKED / ORDERED / unknown, KEEP / REUSE
            for algo in (_lib.ALGO_CHUNKED, _lib.ALGO_ORDERED, 9):
                refused(call(algo=algo), _lib.ERR_UNSUPPORTED_ALGO, "not algorithm")
            for fl in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                refused(call(flags=fl), _lib.ERR_UNSUPPORTED_ALGO, "binning")
            # refusals come before the empty-batch return
            refused(call(B=0, P=0, algo=_lib.ALGO_CHUNKED), _lib.ERR_UNSUPPORTED_ALGO, "not algorithm")
            refused(call(B=0, P=0, K=0), _lib.ERR_INVALID_ARG, "at least one body")
            assert call(flags=_lib.FLAG_COHERENT_POINTS, B=0, P=0) == _lib.OK
        # the forward: TILED, its own pointers, and nothing to do
        refused(f(algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "forward runs on DPR_ALGO_ATOMIC only")
        refused(f(B=0, algo=_lib.ALGO_TILED), _lib.ERR_UNSUPPORTED_ALGO, "ATOMIC only")
        refused(f(values=None), _lib.ERR_INVALID_ARG, "values is NULL")
        refused(f(values=odd), _lib.ERR_INVALID_ARG, "aligned")
        assert f(P=0, values=None, image=None, pts=None, body=None) == _lib.OK
        assert f(B=0, values=None, image=None) == _lib.OK
        # DPR_FLAG_MAX_POSE_GROUP anywhere but the TILED pullback
        for algo in (_lib.ALGO_AUTO, _lib.ALGO_ATOMIC):
            refused(f(algo=algo, flags=MPG(4)), _lib.ERR_UNSUPPORTED_ALGO, "DPR_FLAG_MAX_POSE_GROUP")
            refused(b(algo=algo, flags=MPG(4)), _lib.ERR_UNSUPPORTED_ALGO, "DPR_FLAG_MAX_POSE_GROUP")
        # the pullback's outputs
        refused(b(outs=(None, None, None, None)), _lib.ERR_INVALID_ARG, "every output is NULL")
        refused(b(dv=None), _lib.ERR_INVALID_ARG, "ds_dvalues is NULL")
        refused(b(image=None, outs=(d, None, d, None)), _lib.ERR_INVALID_ARG, "image is NULL")
        refused(b(outs=(d, None, d, None), dv=ctypes.c_void_p(262)), _lib.ERR_INVALID_ARG, "aligned")
        refused(b(outs=(d, d, odd, d)), _lib.ERR_INVALID_ARG, "aligned")
        # DPR_ERR_WORKSPACE on the TILED pullback's ds_dimage: none, one too small, one misaligned -- with the flags of
        # the call in the query -- and the workspace of a group of one does not serve the default group
        for fl in (0, MPG(1)):
            need = query(PULLBACK, _lib.ALGO_TILED, fl, 3, 3, gp, 10, 2, 3)
            assert need not in (0, SIZE_MAX)
            refused(b(algo=_lib.ALGO_TILED, flags=fl), _lib.ERR_WORKSPACE, "workspace")
            refused(b(algo=_lib.ALGO_TILED, flags=fl, ws=d, wsb=need - 1), _lib.ERR_WORKSPACE, "workspace")
            refused(b(algo=_lib.ALGO_TILED, flags=fl, ws=odd, wsb=need), _lib.ERR_WORKSPACE, "256-byte aligned")
        one = query(PULLBACK, _lib.ALGO_TILED, MPG(1), 3, 3, gp, 1000, 2, 3)
        assert one < query(PULLBACK, _lib.ALGO_TILED, 0, 3, 3, gp, 1000, 2, 3)
        refused(b(algo=_lib.ALGO_TILED, P=1000, ws=d, wsb=one), _lib.ERR_WORKSPACE, "workspace")
        refused(b(algo=_lib.ALGO_TILED, P=(1 << 32) - 1, B=1), _lib.ERR_UNSUPPORTED_ALGO, "2^32 - 2")


def test_python_wrappers_raise_without_a_device():
    pts, body = torch.zeros(10, 3), torch.zeros(10, dtype=torch.int64)
    R, t = torch.zeros(4, 2, 2, 3), torch.zeros(4, 2, 2)
    img, dv = torch.zeros(16, 16, 4), torch.zeros(10, 4)
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
    ]
    for kw in bad:
        a = dict(points=pts, body=body, rotation=R, translation=t)
        a.update(kw)
        args = (a["points"], a["body"], a["rotation"], a["translation"])
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.sample_smooth_bodies(img, *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.sample_smooth_bodies_(dv, img, *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.sample_smooth_bodies_pullback_(dv, img, *args)
        with pytest.raises(dpr_amd.DimensionMismatch):
            dpr_amd.sample_smooth_bodies_ad(img, *args)
    with pytest.raises(TypeError):
        dpr_amd.sample_smooth_bodies(img, pts, body.float(), R, t)
    with pytest.raises(ValueError):
        dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, R, t, max_pose_group=40)
    with pytest.raises(ValueError, match="unknown gradient"):
        dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, R, t, need=("weights",))
    with pytest.raises(ValueError, match="at least one"):
        dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, R, t, need=())
    with pytest.raises(ValueError, match="not in need"):
        dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, R, t, need=("image",),
                                               ds_dpoints=torch.zeros(10, 3))
    # consistent shapes on the CPU: the error of `raster`
    for call in (lambda: dpr_amd.sample_smooth_bodies(img, pts, body, R, t),
                 lambda: dpr_amd.sample_smooth_bodies(img[..., 0], pts, body, R[0], t[0]),
                 lambda: dpr_amd.sample_smooth_bodies_(dv, img, pts, body, R, t),
                 lambda: dpr_amd.sample_smooth_bodies_pullback_(dv, img, pts, body, R, t),
                 lambda: dpr_amd.sample_smooth_bodies_ad(img, pts, body, R, t)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
