"""CPU-side checks of the drop-in boundary: libdpr.so loads without a GPU, exports every
symbol include/dpr.h declares, and rejects bad arguments before touching the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpr_amd
from tests.conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "dpr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dpr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = dpr_amd.lib()
    declared = _declared_symbols()
    assert len(declared) >= 12
    for name in declared:
        assert hasattr(L, name), f"libdpr.so does not export {name}"
    assert sorted(dpr_amd._lib.EXPORTS) == declared


def test_version_matches_header():
    text = open(os.path.join(ROOT, "include", "dpr.h")).read()
    ver = int(re.search(r"#define DPR_VERSION (\d+)", text).group(1))
    assert dpr_amd.lib().dpr_version() == ver


def test_status_codes_match_header():
    text = open(os.path.join(ROOT, "include", "dpr.h")).read()
    for name, attr in [("DPR_ERR_UNSUPPORTED_DIMS", "ERR_UNSUPPORTED_DIMS"),
                       ("DPR_ERR_INVALID_ARG", "ERR_INVALID_ARG"),
                       ("DPR_ERR_WORKSPACE", "ERR_WORKSPACE"), ("DPR_ERR_HIP", "ERR_HIP"),
                       ("DPR_ERR_UNSUPPORTED_ALGO", "ERR_UNSUPPORTED_ALGO"),
                       ("DPR_ALGO_ATOMIC", "ALGO_ATOMIC"), ("DPR_ALGO_TILED", "ALGO_TILED"),
                       ("DPR_OP_PULLBACK", "OP_PULLBACK")]:
        val = int(re.search(rf"#define {name} \(?(-?\d+)\)?", text).group(1))
        assert getattr(dpr_amd._lib, attr) == val


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_argument_errors_are_reported_without_a_device(suf):
    """Errors come back as status + dpr_last_error(), nothing is launched
    (reference: @argcheck before launch, src/raster.jl:14-23)."""
    L = dpr_amd.lib()
    grid = np.array([8, 8, 8], dtype=np.int64)
    gp = grid.ctypes.data_as(ctypes.c_void_p)
    fn = getattr(L, f"dpr_raster_{suf}")
    # unsupported dims (1 <= n_in, n_out <= 4 are supported, in any combination)
    rc = fn(None, 2, 5, gp, 10, 1, None, None, None, None, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_DIMS
    assert "unsupported" in dpr_amd._lib.last_error()
    # NULL out
    rc = fn(None, 3, 3, gp, 10, 1, None, None, None, None, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG
    assert "NULL" in dpr_amd._lib.last_error()
    # negative P
    rc = fn(None, 3, 3, gp, -1, 1, None, None, None, None, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG
    # bad grid
    bad = np.array([8, 0, 8], dtype=np.int64)
    rc = fn(None, 3, 3, bad.ctypes.data_as(ctypes.c_void_p), 1, 1, None, None, None, None, None,
            None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG
    pb = getattr(L, f"dpr_raster_pullback_{suf}")
    rc = pb(None, 0, 2, gp, 10, 1, *([None] * 12), None, 0)  # n_in < 1
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_DIMS
    rc = pb(None, 5, 2, gp, 10, 1, *([None] * 12), None, 0)  # n_in > 4
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_DIMS
    rc = pb(None, 1, 2, gp, 10, 1, *([None] * 12), None, 0)  # n_out > n_in is fine: the next check fails
    assert rc == dpr_amd._lib.ERR_INVALID_ARG
    ws = getattr(L, f"dpr_workspace_bytes_{suf}")
    assert ws(0, 0, 3, 3, gp, 1000, 2) != ctypes.c_size_t(-1).value
    assert ws(0, 0, 4, 3, gp, 1000, 2) == 0  # (4-D points: the direct kernels, no workspace)
    assert ws(0, 0, 5, 3, gp, 1000, 2) == ctypes.c_size_t(-1).value
    assert ws(7, 0, 3, 3, gp, 1000, 2) == ctypes.c_size_t(-1).value


def test_comm_entry_points_validate_before_touching_rccl():
    L = dpr_amd.lib()
    small = (ctypes.c_char * 16)()
    assert L.dpr_comm_unique_id(small, 16) == dpr_amd._lib.ERR_INVALID_ARG
    comm = ctypes.c_void_p()
    uid = (ctypes.c_char * 128)()
    assert L.dpr_comm_init(ctypes.byref(comm), 2, 2, uid) == dpr_amd._lib.ERR_INVALID_ARG
    assert L.dpr_comm_init(ctypes.byref(comm), 0, 0, uid) == dpr_amd._lib.ERR_INVALID_ARG
    assert L.dpr_comm_destroy(None) == 0 and L.dpr_comm_world(None) == 0 and L.dpr_comm_rank(None) == -1
    grid = np.array([8, 8, 8], dtype=np.int64)
    rc = L.dpr_raster_pullback_sharded_f32(None, None, 3, 3, grid.ctypes.data_as(ctypes.c_void_p), 10, 1,
                                           *([None] * 12), None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "comm" in dpr_amd._lib.last_error()


def test_host_api_refuses_cpu_tensors():
    """No CPU fallback: the product path must fail loudly off-device."""
    import torch

    pts = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster((5, 5), pts, torch.eye(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.raster_pullback_(torch.zeros(5, 5, dtype=torch.float64), pts,
                                 torch.eye(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


def test_shard_range_is_a_partition():
    L = dpr_amd.lib()
    for B in [0, 1, 5, 8, 9, 64, 513]:
        for world in [1, 2, 3, 8]:
            ranges = [dpr_amd.shard_range(B, r, world) for r in range(world)]
            for r in range(world):  # the C entry point a non-Python host uses agrees
                lo, hi = ctypes.c_int64(), ctypes.c_int64()
                L.dpr_shard_range(B, r, world, ctypes.byref(lo), ctypes.byref(hi))
                assert (lo.value, hi.value) == ranges[r]
            assert ranges[0][0] == 0 and ranges[-1][1] == B
            for (a, b), (c, d) in zip(ranges, ranges[1:]):
                assert b == c
            sizes = [b - a for a, b in ranges]
            assert max(sizes) - min(sizes) <= 1
    # an invalid (rank, world) is an empty range, not a division by zero
    for rank, world in [(0, 0), (0, -1), (3, 2), (-1, 4)]:
        lo, hi = ctypes.c_int64(7), ctypes.c_int64(7)
        L.dpr_shard_range(10, rank, world, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == (0, 0)


def test_chunk_owner_workspace_query_with_no_poses():
    """B == 0 is a valid (empty) batch: the chunk-owner plan must not divide by it."""
    L = dpr_amd.lib()
    grid = (ctypes.c_int64 * 2)(64, 64)
    for op in (0, 1):
        for flags in (0, 4):
            n = L.dpr_workspace_bytes_ex_f32(op, 3, flags, 3, 2, grid, 100_000, 0)
            assert n != ctypes.c_size_t(-1).value and n > 0


def test_auto_algorithm_and_workspace_queries_need_no_device():
    """dpr_resolve_algo / dpr_workspace_bytes_* are pure host arithmetic."""
    import torch

    assert dpr_amd.resolve_algo("raster", (256, 256, 256), 10_000_000, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (256, 256, 256), 10_000_000, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("raster", (8, 8, 8), 1000, 1, 3) == "atomic"
    # batched poses on a grid with few tiles: pose groups repay the forward binning earlier,
    # the direct pullback kernel stays ahead longer (profiles/r01_algo_sweep_batched.txt)
    assert dpr_amd.resolve_algo("raster", (128, 128, 128), 100_000, 16, 3) == "tiled"
    # one pose: the direct kernels up to 2.5e5 points -- on small grids (<= 128^3) only up to 1e5:
    # their atomics are 2x behind there on a clustered cloud (profiles/r03_auto_regret.txt)
    assert dpr_amd.resolve_algo("raster", (256, 256, 256), 100_000, 1, 3) == "atomic"
    assert dpr_amd.resolve_algo("raster", (128, 128, 128), 100_000, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("raster", (128, 128, 128), 50_000, 1, 3) == "atomic"
    # 3-D chunk lists: forward over several poses of a coherent cloud that is sparse on the grid
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 1_000_000, 16, 3, coherent_points=True) == "chunked"
    # (without the flag: sorted inside the call from 16 poses and 2e5 points on)
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 1_000_000, 16, 3) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 1_000_000, 8, 3) == "tiled"
    # dense coherent cloud, two poses or more, >= 1024 owner tiles, 0.4-2 points per voxel: owner-computes forward
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 16, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 2, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 2, 3, coherent_points=True, sharing=True) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 3_000_000, 16, 3, coherent_points=True) == "tiled"    # 0.18 per voxel
    assert dpr_amd.resolve_algo("raster", (128,) * 3, 10_000_000, 16, 3, coherent_points=True) == "tiled"   # 160 tiles
    assert dpr_amd.resolve_algo("raster", (512,) * 3, 50_000_000, 8, 3, coherent_points=True) == "tiled"    # C5: 0.37
    # no flag: 16+ poses of a dense cloud of 3e6+ points are sorted inside the call (owner tiles / direct pullback)
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 32, 3) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 16, 3) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000_000, 16, 3) == "chunked"
    # (a KEEP / REUSE pair of such a batch on a grid with pose groups shares nothing: the flags are dropped first)
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 32, 3, sharing=True) == "chunked"
    assert not dpr_amd.sharing_effective((256,) * 3, 10_000_000, 32, 3)
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 1_000_000, 16, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 500_000, 16, 3, coherent_points=True) == "atomic"
    # (batches of a coherent cloud, 1e6 points and more, fewer than 32 poses: the direct 3-D pullback, pose by pose)
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000_000, 16, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 1_000_000, 4, 3, coherent_points=True) == "chunked"
    # (fewer than 32 poses: direct from P > G / 28 on -- 6e5 points on 256^3)
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 700_000, 4, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 500_000, 4, 3, coherent_points=True) != "chunked"
    assert dpr_amd.resolve_algo("pullback", (128,) * 3, 100_000, 16, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 1_000_000, 64, 3, coherent_points=True) == "atomic"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000_000, 64, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (512, 512), 5_000, 64, 3) == "atomic"
    # many poses onto a 2-D grid: chunk-owned LDS tiles with the pose loop inside
    assert dpr_amd.resolve_algo("pullback", (512, 512), 10_000_000, 64, 3) == "chunked"
    assert dpr_amd.resolve_algo("raster", (512, 512), 10_000_000, 64, 3) == "chunked"
    assert dpr_amd.resolve_algo("raster", (512, 512), 10_000_000, 1, 3) == "tiled"
    # ... a sparse cloud on a large image spreads its chunks too far: the forward stays tiled
    assert dpr_amd.resolve_algo("raster", (1024, 1024), 3_000_000, 8, 3) == "tiled"
    # a keep_binning / reuse_binning pair gets ONE algorithm for both calls, whatever the op
    for P, B, grid in [(1000, 1, (8, 8, 8)), (10_000_000, 1, (256,) * 3), (10_000_000, 64, (512, 512)),
                       (200_000, 16, (128, 128)), (3_000_000, 8, (1024, 1024)), (100_000, 4, (64,) * 3)]:
        pair = {dpr_amd.resolve_algo(op, grid, P, B, 3, sharing=True) for op in ("raster", "pullback")}
        # (a pair that does not share -- AUTO dropped the flags -- may mix: each call works alone)
        assert len(pair) == 1 or not dpr_amd.sharing_effective(grid, P, B, 3), (P, B, grid, pair)
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 1, 3, sharing=True) == "tiled"
    assert dpr_amd.resolve_algo("pullback", (512, 512), 10_000_000, 64, 3, sharing=True) == "chunked"
    # pre-sorted clouds skip the sort: the chunk-owner path pays off from a single pose on
    assert dpr_amd.resolve_algo("raster", (512, 512), 10_000_000, 1, 3, coherent_points=True) == "chunked"
    # one pose of a coherent cloud on a 3-D grid: the pullback gathers directly in cloud order (3-D
    # DPR_ALGO_CHUNKED) and reads nothing a forward could keep -- the pair does not share
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000_000, 1, 3, coherent_points=True) == "chunked"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000_000, 1, 3, coherent_points=True, sharing=True) == "chunked"
    assert dpr_amd.resolve_algo("raster", (256,) * 3, 10_000_000, 1, 3, coherent_points=True, sharing=True) == "tiled"
    assert not dpr_amd.sharing_effective((256,) * 3, 10_000_000, 1, 3, coherent_points=True)
    assert dpr_amd.sharing_effective((256,) * 3, 10_000_000, 1, 3)
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 5_000, 1, 3, coherent_points=True) == "atomic"
    assert dpr_amd.resolve_algo("pullback", (256,) * 3, 10_000, 1, 3, coherent_points=True) == "chunked"
    # more than 32768 tiles: the tiled path works in slabs -- the forward from 1e6 points on, the
    # pullback stays with the direct kernel; a tile layer beyond 16384 tiles -> direct kernels
    assert dpr_amd.resolve_algo("raster", (4096, 4096, 64), 10_000_000, 1, 3) == "tiled"
    assert dpr_amd.resolve_algo("raster", (4096, 4096, 64), 500_000, 1, 3) == "atomic"
    assert dpr_amd.resolve_algo("pullback", (4096, 4096, 64), 10_000_000, 1, 3) == "atomic"
    assert dpr_amd.resolve_algo("raster", (8192, 4096, 32), 10_000_000, 1, 3) == "atomic"
    # ... and a sharing pair there drops its flags (a slab's binning is not kept)
    assert not dpr_amd.sharing_effective((1024,) * 3, 10_000_000, 1, 3)
    assert dpr_amd.workspace_bytes("raster", (8, 8), 100, 1, 2, torch.float64, "atomic") == 0
    small = dpr_amd.workspace_bytes("raster", (256,) * 3, 1_000_000, 1, 3, torch.float32, "tiled")
    big = dpr_amd.workspace_bytes("raster", (256,) * 3, 10_000_000, 1, 3, torch.float32, "tiled")
    assert 0 < small < big < 10_000_000 * 64
    assert dpr_amd.workspace_bytes("pullback", (256,) * 3, 10_000_000, 1, 3, torch.float32, "tiled") == big
    f64 = dpr_amd.workspace_bytes("raster", (256,) * 3, 10_000_000, 1, 3, torch.float64, "tiled")
    assert f64 > big
    assert dpr_amd.workspace_bytes("raster", (256,) * 3, 10_000_000, 4, 3, torch.float32, "chunked") > 0
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.workspace_bytes("raster", (8, 8, 8, 8), 10, 1, 3, torch.float32, "tiled")


@pytest.mark.parametrize("suf,ctype", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_workspace_and_flag_errors_precede_any_launch(suf, ctype):
    """A too-small workspace, or binning flags on the wrong algorithm / batch size, are
    rejected on the host (dummy non-NULL pointers are never dereferenced)."""
    L = dpr_amd.lib()
    grid = np.array([64, 64, 64], dtype=np.int64)
    gp = grid.ctypes.data_as(ctypes.c_void_p)
    dummy = (ctypes.c_char * 1024)()
    d = ctypes.c_void_p((ctypes.addressof(dummy) + 255) & ~255)  # 256-byte aligned
    fn = getattr(L, f"dpr_raster_ex_{suf}")
    # misaligned workspace / data pointers would fault on the device: refused
    odd = ctypes.c_void_p(d.value + 4)
    rc = fn(None, dpr_amd._lib.ALGO_TILED, 0, 3, 3, gp, 1000, 1, d, d, d, d, None, None, None, odd,
            1 << 30)
    assert rc == dpr_amd._lib.ERR_WORKSPACE and "aligned" in dpr_amd._lib.last_error()
    rc = fn(None, dpr_amd._lib.ALGO_ATOMIC, 0, 3, 3, gp, 1000, 1, ctypes.c_void_p(d.value + 2), d,
            d, d, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "aligned" in dpr_amd._lib.last_error()
    # every data pointer is checked, not only out / points
    rc = fn(None, dpr_amd._lib.ALGO_ATOMIC, 0, 3, 3, gp, 1000, 1, d, d, ctypes.c_void_p(d.value + 2),
            d, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "aligned" in dpr_amd._lib.last_error()
    rc = fn(None, dpr_amd._lib.ALGO_ATOMIC, 0, 3, 3, gp, 1000, 1, d, d, d, d, None, None,
            ctypes.c_void_p(d.value + 1), None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "aligned" in dpr_amd._lib.last_error()
    pbx = getattr(L, f"dpr_raster_pullback_ex_{suf}")
    rc = pbx(None, dpr_amd._lib.ALGO_ATOMIC, 0, 3, 3, gp, 1000, 1, *([d] * 4), None, None, d,
             ctypes.c_void_p(d.value + 2), *([d] * 4), None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "aligned" in dpr_amd._lib.last_error()
    # a workspace query for a call that TILED would refuse fails too
    wsq = getattr(L, f"dpr_workspace_bytes_{suf}")
    assert wsq(0, dpr_amd._lib.ALGO_TILED, 3, 3, gp, 1 << 32, 1) == ctypes.c_size_t(-1).value
    # more than 32768 tiles: processed in slabs of tile layers (supported, no binning to keep);
    # a single tile LAYER beyond 16384 tiles is not
    big = np.array([4096, 4096, 64], dtype=np.int64)
    bigp = big.ctypes.data_as(ctypes.c_void_p)
    assert 0 < wsq(0, dpr_amd._lib.ALGO_TILED, 3, 3, bigp, 1000, 1) < ctypes.c_size_t(-1).value
    assert getattr(L, f"dpr_workspace_bytes_ex_{suf}")(
        0, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_KEEP_BINNING, 3, 3, bigp, 1000, 1) == ctypes.c_size_t(-1).value
    huge = np.array([8192, 4096, 32], dtype=np.int64)
    assert wsq(0, dpr_amd._lib.ALGO_TILED, 3, 3, huge.ctypes.data_as(ctypes.c_void_p), 1000, 1) == ctypes.c_size_t(-1).value
    # pose-group cap: smaller workspace, same call otherwise
    wsx = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    g2 = np.array([512, 512], dtype=np.int64)
    g2p = g2.ctypes.data_as(ctypes.c_void_p)
    full = wsx(0, dpr_amd._lib.ALGO_TILED, 0, 3, 2, g2p, 1_000_000, 8)
    capped = wsx(0, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.flag_max_pose_group(1), 3, 2, g2p, 1_000_000, 8)
    assert 0 < capped < full / 3 and full == wsq(0, dpr_amd._lib.ALGO_TILED, 3, 2, g2p, 1_000_000, 8)
    # the residual pullback needs a target and has no chunked variant
    rp = getattr(L, f"dpr_raster_residual_pullback_ex_{suf}")
    rc = rp(None, dpr_amd._lib.ALGO_ATOMIC, 0, 3, 3, gp, 1000, 1, d, None, 2.0, d, d, d, None, None,
            None, *([d] * 6), None, 0)
    assert rc == dpr_amd._lib.ERR_INVALID_ARG and "target" in dpr_amd._lib.last_error()
    rc = rp(None, dpr_amd._lib.ALGO_CHUNKED, 0, 3, 3, gp, 1000, 1, d, d, 2.0, d, d, d, None, None,
            None, *([d] * 6), d, 1 << 30)
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_ALGO
    # tiled needs a workspace
    rc = fn(None, dpr_amd._lib.ALGO_TILED, 0, 3, 3, gp, 1000, 1, d, d, d, d, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_WORKSPACE and "workspace" in dpr_amd._lib.last_error()
    rc = fn(None, dpr_amd._lib.ALGO_TILED, 0, 3, 3, gp, 1000, 1, d, d, d, d, None, None, None, d, 64)
    assert rc == dpr_amd._lib.ERR_WORKSPACE
    # keep / reuse flags: tiled or chunked only
    rc = fn(None, dpr_amd._lib.ALGO_ATOMIC, dpr_amd._lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 1, d, d,
            d, d, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_ALGO
    # tiled with B > 1: every pose keeps its own binning (the per-pose part of the workspace is
    # laid out B times, pose groups are off): another layout and size than the same call without
    # the flag, the same for the two calls of a pair, and checked before any launch
    wsx = getattr(L, f"dpr_workspace_bytes_ex_{suf}")
    one = wsx(0, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 1)
    kept = wsx(0, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 3)
    assert kept > one
    assert wsx(1, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_REUSE_BINNING, 3, 3, gp, 1000, 3) == kept
    rc = fn(None, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_KEEP_BINNING, 3, 3, gp, 1000, 3, d, d,
            d, d, None, None, None, d, kept - 256)
    assert rc == dpr_amd._lib.ERR_WORKSPACE and "workspace" in dpr_amd._lib.last_error()
    pb = getattr(L, f"dpr_raster_pullback_ex_{suf}")
    rc = pb(None, dpr_amd._lib.ALGO_TILED, dpr_amd._lib.FLAG_REUSE_BINNING, 3, 3, gp, 1000, 3,
            *([d] * 4), None, None, *([d] * 6), d, kept - 256)
    assert rc == dpr_amd._lib.ERR_WORKSPACE
    # unknown algorithm id
    rc = fn(None, 77, 0, 3, 3, gp, 1000, 1, d, d, d, d, None, None, None, None, 0)
    assert rc == dpr_amd._lib.ERR_UNSUPPORTED_ALGO
    # the sort utility validates too
    srt = getattr(L, f"dpr_sort_points_{suf}")
    assert srt(None, 4, 10, d, d, d, None, None, d, 1 << 20) == dpr_amd._lib.ERR_UNSUPPORTED_DIMS
    assert srt(None, 3, 10, d, d, d, d, None, d, 1 << 20) == dpr_amd._lib.ERR_INVALID_ARG
    dummy2 = (ctypes.c_char * 1024)()
    d2 = ctypes.c_void_p((ctypes.addressof(dummy2) + 255) & ~255)
    assert srt(None, 3, 10, d, d2, d, None, None, d, 8) == dpr_amd._lib.ERR_WORKSPACE


# ------------------------------------------------------------------ code-object gates (no GPU needed)
# Kernels that may use scratch, as (regex on the demangled name, bytes of scratch allowed, why).  Everything
# else in libdpr.so must have .vgpr_spill_count == 0 and .private_segment_fixed_size == 0: a spill in
# a record loop is a silent 10-30 % (round 4: `k_bin_local` 62 -> 150 us when it went from 60 to 128
# VGPRs + scratch).  Budgets are what the round-6 build needs: a larger number fails the test too.
SCRATCH_ALLOWED = [
    (r"rocprim::", 128, "third-party radix sort (private arrays, no VGPR spills)"),
    (r"dpr::k_co_splat_wide<float, 3, (true|false)>", 84,
     "cold path of the 2-D chunk-owner forward (footprints that outgrow the tile): 16 contributions per thread "
     "kept across row bands; recomputing them instead measured slower (experiments/r05_wide_splat_recompute...)"),
    (r"dpr::k_co_splat_wide<float, 2, (true|false)>", 48, "as above, 2-D -> 2-D"),
    (r"dpr::k_co_splat_wide<double, 3, true>", 28, "as above, fp64 with point weights"),
    (r"dpr::k_co_gather<double, 3, true>", 36, "fp64 chunk-owner pullback with point weights at the 128-VGPR cap of a "
                                               "1024-thread workgroup"),
    (r"dpr::k_scatter_wc<float, 3, 3, (true|false), 4096, true, (true|false)>", 76,
     "pose-GROUP variants (batches on 3-D grids of <= 256 tiles): the sub-chunk's points live across the pose loop"),
    (r"dpr::k_bin_local<float, 3, 3, (true|false), 4096, false, false, 1024, true>", 68,
     "local binning of a BATCH (points live across the pose loop); the single-pose variant is clean"),
    (r"dpr::k_tile_gather_runs<double, 3, 3, true, true, true, true>", 12,
     "fp64 run-walking pullback tile kernel with point weights at the 128-VGPR cap"),
]


def test_scratch_use_matches_the_allow_list():
    """Zero-scratch gate: llvm-readelf --notes on the gfx950 code objects inside libdpr.so (no GPU)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources, short

    ks = kernel_resources()
    assert len(ks) > 300, "libdpr.so should hold several hundred kernel instantiations"
    bad, used = [], set()
    for k in ks:
        if not (k["vgpr_spill"] or k["scratch"]):
            continue
        name = short(k["demangled"])
        for i, (pat, budget, _why) in enumerate(SCRATCH_ALLOWED):
            if re.search(pat, k["demangled"]):
                used.add(i)
                if k["scratch"] > budget:
                    bad.append(f"{name}: {k['scratch']} B of scratch > allowed {budget}")
                break
        else:
            bad.append(f"{name}: {k['vgpr_spill']} spilled VGPRs, {k['scratch']} B of scratch")
    assert not bad, "\n".join(bad)
    stale = [SCRATCH_ALLOWED[i][0] for i in range(len(SCRATCH_ALLOWED)) if i not in used]
    assert not stale, f"allow-list entries no kernel needs any more: {stale}"
    # the kernels of the headline configuration (C3, one pose, fp32) are not on the list at all
    for k in ks:
        if re.search(r"dpr::(k_count|k_tile_splat|k_tile_gather|k_unpermute|k_halo_gather|k_own_\w+)<float, 3", k["demangled"]) \
                or re.search(r"dpr::k_scatter_wc<float, 3, 3, false, 4096, false", k["demangled"]):
            assert k["vgpr_spill"] == 0 and k["scratch"] == 0, short(k["demangled"])


# Kernels two objects may both hold: dpr_chunkown.o launches the background fill and the grid sum itself, beside
# the instantiations dpr_api.o keeps for every other caller (fill_background / grid_sum of csrc/dpr_host.h).
TWICE_ALLOWED = {f"dpr::{k}<{t}>" for k in ("k_fill_background", "k_grid_sum") for t in ("float", "double")}


def test_no_kernel_is_compiled_into_two_objects():
    """Every kernel name occurs once among the code objects of libdpr.so (one per translation unit), TWICE_ALLOWED
    excepted: a helper that launches a shared kernel is defined in one unit and declared in csrc/dpr_host.h, so a
    new op family calls it and does not instantiate the kernel again (no GPU)."""
    import collections
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources, short

    ks = kernel_resources()
    count = collections.Counter(k["name"] for k in ks)
    assert len(count) > 300, "libdpr.so should hold several hundred kernel instantiations"
    demangled = {k["name"]: short(k["demangled"]) for k in ks}
    twice = {demangled[n]: c for n, c in count.items() if c > 1}
    assert twice == {name: 2 for name in TWICE_ALLOWED}, twice


# ------------------------------------------------------------------ DPR_ALGO_AUTO, pinned
def _auto_regret(rows, n_in):
    worst = {"raster": (1.0, None), "pullback": (1.0, None)}
    for r in rows:
        kw = dict(coherent_points=True) if r["order"] == "coherent" else {}
        for op in ("raster", "pullback"):
            auto = dpr_amd.resolve_algo(op, tuple(r["grid"]), r["P"], r["B"], n_in, **kw)
            assert auto in r[op], f"AUTO picks {auto} where the table has no time: {r}"
            regret = r[op][auto] / min(r[op].values())
            if regret > worst[op][0]:
                worst[op] = (regret, r)
    return worst


def test_auto_stays_within_its_measured_regret():
    """`resolve_algo` is ~250 lines of thresholds fitted to measured tables; the table of round 5 (336 shapes
    x 2 operations, three cloud distributions, both point orders; tools/auto_regret.py on one MI355X) is
    committed as tests/golden/auto_regret_r05.json and AUTO is re-evaluated against it on the host: the
    worst ratio t(AUTO) / t(best) must stay where profiles/r05_auto_regret.txt left it (1.59 forward, 1.43
    pullback).  A threshold edit that sends a measured shape to a slower algorithm fails here."""
    import json
    tab = json.load(open(os.path.join(ROOT, "tests", "golden", "auto_regret_r05.json")))
    assert len(tab["rows"]) == 336
    worst = _auto_regret(tab["rows"], tab["n_in"])
    assert worst["raster"][0] <= 1.60, worst["raster"]
    assert worst["pullback"][0] <= 1.45, worst["pullback"]


def test_auto_choice_for_the_baseline_configs_and_the_readme_shapes():
    """The documented choices: every BASELINE.json config and the reference's published
    shapes (README.md:189-193: 1e4 / 1e5 points x 64 images -> 128^2 / 1024^2, and 1e5 points -> 1024^3)."""
    ra = dpr_amd.resolve_algo
    # C1: 1k 2-D points -> 5x5: direct kernels
    assert ra("raster", (5, 5), 1000, 1, 2) == "atomic" and ra("pullback", (5, 5), 1000, 1, 2) == "atomic"
    # C2 / C3: single pose, dense cloud on a 3-D grid in any order: tiled (also as a KEEP / REUSE pair)
    for P, g in ((1_000_000, (128,) * 3), (10_000_000, (256,) * 3)):
        assert ra("raster", g, P, 1, 3) == "tiled" and ra("pullback", g, P, 1, 3) == "tiled"
        assert ra("raster", g, P, 1, 3, sharing=True) == "tiled"
    # C3 on a cloud flagged coherent: the pullback gathers directly (nothing to share with the forward)
    assert ra("pullback", (256,) * 3, 10_000_000, 1, 3, coherent_points=True) == "chunked"
    assert not dpr_amd.sharing_effective((256,) * 3, 10_000_000, 1, 3, coherent_points=True)
    # C4: 10 M points -> 512^2, 64 poses per GPU (and the 512-pose job): chunk-owner tiles
    for B in (64, 512):
        assert ra("raster", (512, 512), 10_000_000, B, 3) == "chunked"
        assert ra("pullback", (512, 512), 10_000_000, B, 3) == "chunked"
    # C5: 50 M points -> 512^3, 8 poses per GPU: tiled forward; the pullback of a cloud in any order sorts
    # inside the call and gathers directly (>= 8 poses of >= 1e7 points)
    assert ra("raster", (512,) * 3, 50_000_000, 8, 3) == "tiled"
    assert ra("pullback", (512,) * 3, 50_000_000, 8, 3) == "chunked"
    # the README's timing table: 1e5 points x 64 poses
    for P in (10_000, 100_000):
        assert ra("raster", (128, 128), P, 64, 3) == "chunked"
        assert ra("pullback", (128, 128), P, 64, 3) in ("atomic", "chunked")
        assert ra("raster", (1024, 1024), P, 64, 3) in ("chunked", "atomic")
    assert ra("raster", (1024,) * 3, 100_000, 1, 3) == "atomic"  # (a sparse cloud on a huge grid: direct atomics)
    assert ra("pullback", (1024,) * 3, 100_000, 1, 3) == "atomic"
    # the residual pullback never resolves to the 3-D direct kernels
    assert ra("residual_pullback", (256,) * 3, 10_000_000, 1, 3, coherent_points=True) == "tiled"
    assert ra("residual_pullback", (256,) * 3, 10_000_000, 16, 3) == "tiled"
