"""DPR_ALGO_ORDERED at the ABI: constants, workspace queries, limits, flag and workspace errors, the refusals of
the other op families, and DPR_ALGO_AUTO unchanged.  No GPU: every call here returns before anything is launched
(dummy non-NULL pointers are never dereferenced)."""
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
SIZE_MAX = ctypes.c_size_t(-1).value
PAIRS = [(i, o) for i in range(1, 5) for o in range(1, 5)]
SUFS = ["f32", "f64"]
# the extended grid (n_d + 1 per axis) of this one has 2 * 2 * 32769^2 > 2^32 cells; its 2^30 voxels are a valid grid
BEYOND = (1, 1, 32768, 32768)


def _header():
    return open(os.path.join(ROOT, "include", "dpr.h")).read()


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def d():
    buf = (ctypes.c_char * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    p._keep = buf
    return p


def test_constants_and_version_match_the_header():
    h = _header()
    assert int(re.search(r"#define DPR_ALGO_ORDERED (\d+)", h).group(1)) == _lib.ALGO_ORDERED == 4
    assert _lib.ALGOS["ordered"] == _lib.ALGO_ORDERED
    assert dpr_amd.lib().dpr_version() == int(re.search(r"#define DPR_VERSION (\d+)", h).group(1)) == 110
    for name in ("DPR_ORDERED_POINT_CHUNK", "DPR_ORDERED_CELL_CHUNK"):
        assert int(re.search(rf"#define {name} (\d+)", h).group(1)) % 256 == 0
    stages = dpr_amd._pkg.timing.STAGES
    assert stages[("raster", "ordered")] and stages[("pullback", "ordered")]


@pytest.mark.parametrize("suf", SUFS)
def test_workspace_query_answers_for_every_pair_and_op(suf):
    ws = getattr(dpr_amd.lib(), f"dpr_workspace_bytes_ex_{suf}")
    for n_in, n_out in PAIRS:
        a, gp = _g((8,) * n_out)
        for op in (_lib.OP_RASTER, _lib.OP_PULLBACK, _lib.OP_RESIDUAL_PULLBACK):
            sizes = [ws(op, _lib.ALGO_ORDERED, 0, n_in, n_out, gp, P, 3) for P in (0, 1, 255, 5000, 100_000, 10_000_000)]
            assert SIZE_MAX not in sizes, (n_in, n_out, op)
            assert sizes[0] <= 4096, "P = 0 needs (next to) no workspace"
            assert sizes == sorted(sizes), "non-decreasing in P"
            assert sizes[-1] > sizes[0]
            # COHERENT_POINTS / MAX_POSE_GROUP / NO_POINT_WEIGHT_GRAD: accepted, the same size
            for fl in (_lib.FLAG_COHERENT_POINTS, _lib.flag_max_pose_group(4), _lib.FLAG_NO_POINT_WEIGHT_GRAD):
                assert ws(op, _lib.ALGO_ORDERED, fl, n_in, n_out, gp, 5000, 3) == sizes[3]
        fwd = {ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, 0, n_in, n_out, gp, 5000, B) for B in (1, 2, 7, 64)}
        assert len(fwd) == 1, "the forward's workspace does not depend on B"
        # O(P) + O(G): 16 P + the sort's temporary storage + the start table
        big = ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, 0, n_in, n_out, gp, 10_000_000, 1)
        assert big < 10_000_000 * 40
    assert dpr_amd.workspace_bytes("raster", (256,) * 3, 10_000_000, 1, 3, torch.float32, "ordered") < 10_000_000 * 40
    # the pullback's partials stay modest at 1e7 points x 64 poses
    assert dpr_amd.workspace_bytes("pullback", (256,) * 3, 10_000_000, 64, 3, torch.float32, "ordered") < 64 << 20


@pytest.mark.parametrize("suf", SUFS)
def test_key_limit_is_refused(suf, d):
    L = dpr_amd.lib()
    ws = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    a, gp = _g(BEYOND)
    for op in (_lib.OP_RASTER, _lib.OP_PULLBACK, _lib.OP_RESIDUAL_PULLBACK):
        assert ws(op, _lib.ALGO_ORDERED, 0, 3, 4, gp, 1000, 1) == SIZE_MAX
        assert ws(op, _lib.ALGO_ATOMIC, 0, 3, 4, gp, 1000, 1) == 0  # (a valid grid for the others)
    rc = getattr(L, f"dpr_raster_ex_{suf}")(None, _lib.ALGO_ORDERED, 0, 3, 4, gp, 1000, 1, d, d, d, d, None, None, None,
                                           d, 1 << 40)
    assert rc == _lib.ERR_UNSUPPORTED_ALGO and "ORDERED" in _lib.last_error()
    rc = getattr(L, f"dpr_raster_pullback_ex_{suf}")(None, _lib.ALGO_ORDERED, 0, 3, 4, gp, 1000, 1, *([d] * 4), None,
                                                    None, *([d] * 6), d, 1 << 40)
    assert rc == _lib.ERR_UNSUPPORTED_ALGO
    # P beyond 2^32 - 2
    a, gp = _g((8, 8, 8))
    assert ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, 0, 3, 3, gp, (1 << 32) - 1, 1) == SIZE_MAX
    assert ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, 0, 3, 3, gp, (1 << 32) - 2, 1) != SIZE_MAX


@pytest.mark.parametrize("suf", SUFS)
def test_flag_and_workspace_errors_precede_any_launch(suf, d):
    L = dpr_amd.lib()
    a, gp = _g((64, 64, 64))
    fn = getattr(L, f"dpr_raster_ex_{suf}")
    pb = getattr(L, f"dpr_raster_pullback_ex_{suf}")
    rp = getattr(L, f"dpr_raster_residual_pullback_ex_{suf}")
    ws = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    # KEEP / REUSE: nothing to keep, as for DPR_ALGO_ATOMIC
    rc = fn(None, _lib.ALGO_ORDERED, _lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 1, d, d, d, d, None, None, None, d, 1 << 30)
    assert rc == _lib.ERR_UNSUPPORTED_ALGO
    rc = pb(None, _lib.ALGO_ORDERED, _lib.FLAG_REUSE_BINNING, 3, 3, gp, 1000, 1, *([d] * 4), None, None, *([d] * 6), d,
            1 << 30)
    assert rc == _lib.ERR_UNSUPPORTED_ALGO
    assert ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, _lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 1) == SIZE_MAX
    assert ws(_lib.OP_PULLBACK, _lib.ALGO_ORDERED, _lib.FLAG_REUSE_BINNING, 3, 3, gp, 1000, 1) == SIZE_MAX
    # dpr_resolve_flags_ex is about AUTO and unchanged
    assert L.dpr_resolve_flags_ex(_lib.OP_RASTER, _lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 1) == 0
    # a missing or short workspace
    need_f = ws(_lib.OP_RASTER, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2)
    need_b = ws(_lib.OP_PULLBACK, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2)
    need_r = ws(_lib.OP_RESIDUAL_PULLBACK, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2)
    assert need_f > 0 and need_b > 0 and need_r == need_b
    for ptr, size in ((None, 0), (d, need_f - 256)):
        rc = fn(None, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2, d, d, d, d, None, None, None, ptr, size)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    for ptr, size in ((None, 0), (d, need_b - 256)):
        rc = pb(None, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2, *([d] * 4), None, None, *([d] * 6), ptr, size)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
        rc = rp(None, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2, d, d, 2.0, d, d, d, None, None, d, *([d] * 6), ptr, size)
        assert rc == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    # a misaligned workspace
    rc = fn(None, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2, d, d, d, d, None, None, None, ctypes.c_void_p(d.value + 4),
            1 << 30)
    assert rc == _lib.ERR_WORKSPACE and "aligned" in _lib.last_error()
    # the residual needs its target whatever the algorithm
    rc = rp(None, _lib.ALGO_ORDERED, 0, 3, 3, gp, 1000, 2, d, None, 2.0, d, d, d, None, None, None, *([d] * 6), d, 1 << 30)
    assert rc == _lib.ERR_INVALID_ARG and "target" in _lib.last_error()


@pytest.mark.parametrize("suf", SUFS)
def test_other_op_families_refuse_the_algorithm(suf, d):
    L = dpr_amd.lib()
    A = _lib.ALGO_ORDERED
    big = 1 << 30
    for n_in, n_out in [(3, 3), (2, 2), (3, 2), (1, 1), (2, 3), (4, 4)]:
        a, gp = _g((16,) * n_out)
        head = (None, A, 0, n_in, n_out, gp, 1000, 2)
        for op in (_lib.OP_RASTER, _lib.OP_PULLBACK):
            assert getattr(L, f"dpr_workspace_bytes_channels_ex_{suf}")(op, A, 0, n_in, n_out, gp, 1000, 2, 3) == SIZE_MAX
            assert getattr(L, f"dpr_workspace_bytes_sample_ex_{suf}")(op, A, 0, n_in, n_out, gp, 1000, 2) == SIZE_MAX
            assert getattr(L, f"dpr_workspace_bytes_clouds_ex_{suf}")(op, A, 0, n_in, n_out, gp, 1000, 2) == SIZE_MAX
        assert getattr(L, f"dpr_workspace_bytes_jvp_ex_{suf}")(A, 0, n_in, n_out, gp, 1000, 2, 2) == SIZE_MAX
        U = _lib.ERR_UNSUPPORTED_ALGO
        assert getattr(L, f"dpr_raster_channels_ex_{suf}")(*head, 3, *([d] * 4), None, None, None, d, big) == U
        assert getattr(L, f"dpr_raster_pullback_channels_ex_{suf}")(*head, 3, *([d] * 4), None, None, *([d] * 6), d, big) == U
        assert getattr(L, f"dpr_sample_ex_{suf}")(*head, *([d] * 5), d, big) == U
        assert getattr(L, f"dpr_sample_pullback_ex_{suf}")(*head, *([d] * 9), d, big) == U
        assert getattr(L, f"dpr_raster_jvp_ex_{suf}")(*head, 2, *([d] * 4), None, None, *([d] * 6), d, big) == U
        assert getattr(L, f"dpr_raster_clouds_ex_{suf}")(*head, d, d, d, d, None, None, None, d, big) == U
        assert getattr(L, f"dpr_raster_pullback_clouds_ex_{suf}")(*head, *([d] * 4), None, None, *([d] * 6), d, big) == U


def test_auto_is_unchanged_and_never_ordered():
    L = dpr_amd.lib()
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "auto_regret_r05.json")))
    was = json.load(open(os.path.join(ROOT, "tests", "golden", "auto_answers_0_1_9.json")))
    assert len(rows["rows"]) == len(was["rows"]) == 336 and rows["n_in"] == was["n_in"]
    names = {v: k for k, v in _lib.ALGOS.items()}
    for r, w in zip(rows["rows"], was["rows"]):
        assert (r["grid"], r["P"], r["B"], r["order"]) == (w["grid"], w["P"], w["B"], w["order"])
        a, gp = _g(r["grid"])
        base = _lib.FLAG_COHERENT_POINTS if r["order"] == "coherent" else 0
        for op, opc in (("raster", _lib.OP_RASTER), ("pullback", _lib.OP_PULLBACK)):
            got = L.dpr_resolve_algo_ex(opc, base, rows["n_in"], len(r["grid"]), gp, r["P"], r["B"])
            assert got in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED, _lib.ALGO_CHUNKED) and names[got] == w[op], (r, op)
            for extra in (_lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING):
                got = L.dpr_resolve_algo_ex(opc, base | extra, rows["n_in"], len(r["grid"]), gp, r["P"], r["B"])
                assert got in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED, _lib.ALGO_CHUNKED)
        got = L.dpr_resolve_algo_ex(_lib.OP_RESIDUAL_PULLBACK, base, rows["n_in"], len(r["grid"]), gp, r["P"], r["B"])
        assert got in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED, _lib.ALGO_CHUNKED)
    clouds = json.load(open(os.path.join(ROOT, "tests", "golden", "clouds_auto.json")))
    for row in clouds["shapes"]:
        a, gp = _g(row["grid"])
        for op, want in row["auto"].items():
            opc = {"raster": _lib.OP_RASTER, "pullback": _lib.OP_PULLBACK}[op]
            if row.get("dtype", "float32") == "float32":
                got = L.dpr_resolve_algo_clouds(opc, row["n_in"], len(row["grid"]), gp, row["P"], row["B"])
                assert got == _lib.ALGOS[want] and got != _lib.ALGO_ORDERED
            # the single-cloud AUTO on the same shape
            got = L.dpr_resolve_algo_ex(opc, 0, row["n_in"], len(row["grid"]), gp, row["P"], row["B"])
            assert got in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED, _lib.ALGO_CHUNKED)
    # all 16 pairs: AUTO never answers 4
    for n_in, n_out in PAIRS:
        a, gp = _g((32,) * n_out)
        for op in (0, 1, 2):
            for P, B in ((10, 1), (100_000, 1), (1_000_000, 16)):
                assert L.dpr_resolve_algo_ex(op, 0, n_in, n_out, gp, P, B) in (1, 2, 3)


def test_python_surface_accepts_the_name():
    assert dpr_amd.workspace_bytes("raster", (8, 8, 8), 0, 3, 3, torch.float32, "ordered") == 0
    for op in ("raster", "pullback", "residual_pullback"):
        assert dpr_amd.workspace_bytes(op, (7, 9, 5), 5000, 3, 3, torch.float64, "ordered") > 0
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes("raster", BEYOND, 10, 1, 3, torch.float32, "ordered")
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes("raster", (8, 8, 8), 10, 1, 3, torch.float32, "ordered", sharing=True)
