"""The workspace contract of include/dpr.h, row by row of tests/workspace_cases.py: the initial contents of the
workspace do not matter, and a call writes only inside [workspace, workspace + workspace_bytes).

Every row runs on the interior view buf[4096 : 4096 + need] of a uint8 buffer of need + 8192 bytes whose two guard
bands hold 0xA5: the library is handed exactly `need` bytes at a 256-byte aligned address (the Python layer passes the
view's own size), and an overrun lands in memory this test owns.  Three workspace contents:
  zeros   what a first allocation of a new process holds;
  stale   what a call of the same row with another cloud, other poses and other images left behind (every index,
          count and key in it is in range for the shape);
  ones    every byte 0xFF: NaN as a float, the all-ones key, the largest count -- only for rows whose pieces the
          audit of DESIGN.md 4.18 found written before they are read (Row.poison).
After each call both guard bands are unchanged byte for byte; every output (allocated here and filled with NaN, so
"fully overwritten" is held too) is finite and matches the reference of the family's own test module at that
module's tolerance; and the outputs that include/dpr.h's SUMMATION ORDER tables call bit-reproducible run to run
(Row.exact quotes the line) are torch.equal to those of the zeros run.  For the KEEP / REUSE row the buffer is
filled before the first forward only.
"""
import pytest
import torch

import dpr_amd
from tests.test_parity_gpu import assert_close
from tests.workspace_cases import (FAMILIES, FLAGS, PULLBACK_FIELDS, TABLE, need_bytes, problem, reference, row_id,
                                   tolerance)

gpu = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
CASES = [(row, dt) for row in TABLE for dt in row.dtypes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dpr_amd.lib()
    return torch.device("cuda:0")


def run_row(row, inp, p, dev, ws):
    """One call of the row (the pair row: four) on workspace `ws`; name -> output tensor."""
    fam = FAMILIES[row.family]
    if row.op != "pair":
        out = fam.outputs(row.op, p, dev)
        fam.call(row.op, row.algo, FLAGS[row.flags], inp, out, ws)
        return out
    poses = fam.poses(inp)
    kw = dict(algo=row.algo, workspace=ws)
    pb = lambda o: {f"ds_d{k}": o[k] for k in PULLBACK_FIELDS}
    fwd, fwd2 = fam.outputs("raster", p, dev), fam.outputs("raster", p, dev)
    o_pb, o_res = fam.outputs("pullback", p, dev), fam.outputs("residual_pullback", p, dev)
    dpr_amd.raster_(fwd["out"], *poses, keep_binning=True, **kw)
    dpr_amd.raster_pullback_(inp["g"], *poses, reuse_binning=True, **pb(o_pb), **kw)
    dpr_amd.raster_(fwd2["out"], *poses, keep_binning=True, **kw)  # (the pullback has consumed the first binning)
    dpr_amd.raster_residual_pullback_(inp["out_img"], inp["target"], *poses, scale=2.0, loss=o_res["loss"],
                                      reuse_binning=True, **pb(o_res), **kw)
    out = dict(fwd, **{"second/out": fwd2["out"]})
    out.update({f"pullback/{k}": v for k, v in o_pb.items()})
    out.update({f"residual_pullback/{k}": v for k, v in o_res.items()})
    return out


def expected(row, dt, seed=0):
    shape = (row.family, row.n_in, row.grid, row.P, row.B, dt, seed)
    ref = lambda op: reference(shape[0], op, *shape[1:])
    if row.op != "pair":
        return ref(row.op)
    out = dict(ref("raster"), **{"second/out": ref("raster")["out"]})
    out.update({f"pullback/{k}": v for k, v in ref("pullback").items()})
    out.update({f"residual_pullback/{k}": v for k, v in ref("residual_pullback").items()})
    return out


@gpu
@pytest.mark.parametrize("row,dt", CASES, ids=[row_id(r, d) for r, d in CASES])
def test_initial_contents_do_not_matter_and_nothing_is_written_outside(dev, row, dt):
    fam = FAMILIES[row.family]
    shape = (row.family, row.n_in, row.grid, row.P, row.B, dt)
    p, other = problem(*shape, 0), problem(*shape, 1)
    inp, inp_other = fam.to_device(p, dev), fam.to_device(other, dev)
    need = need_bytes(row, dt)
    assert need > 0, "a row of the table needs a workspace"
    buf = torch.full((need + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    band = torch.full((GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() * ws.element_size() == need
    ref = expected(row, dt)
    first = None
    for pattern in ("zeros", "stale", "ones"):
        if pattern == "zeros":
            ws.zero_()
        elif pattern == "stale":
            run_row(row, inp_other, other, dev, ws)
        elif not row.poison:
            continue
        else:
            ws.fill_(0xFF)
        out = run_row(row, inp, p, dev, ws)
        torch.cuda.synchronize()
        assert torch.equal(buf[:GUARD], band), f"{pattern}: bytes in front of the workspace were overwritten"
        assert torch.equal(buf[GUARD + need:], band), f"{pattern}: bytes behind the {need} queried were overwritten"
        assert set(out) == set(ref)
        for name, got in out.items():
            field = name.split("/")[-1]
            assert bool(torch.isfinite(got).all()), f"{pattern}: {name} holds NaN / Inf (or was not overwritten)"
            assert_close(got, ref[name], tolerance(row.family, dt, field), f"{pattern}: {name}")
        if first is None:
            first = {k: v.clone() for k, v in out.items()}
            continue
        for name, got in out.items():
            dtypes, quote = row.exact.get(name.split("/")[-1], ((), ""))
            if dt in dtypes:
                assert torch.equal(got, first[name]), \
                    f"{pattern}: {name} differs from the run on a zeroed workspace, max |d| = " \
                    f"{float((got.double() - first[name].double()).abs().max()):.3e}; include/dpr.h: {quote}"


def test_the_table_runs_every_row_in_both_element_types_where_it_has_them():
    """(CPU)  fp32 and fp64 wherever the path has both: the one exception is the per-pose cloud forward on
    DPR_ALGO_CHUNKED, whose workspace (the per-pose weight keys of the fixed-point scale) exists for fp32 only."""
    for row in TABLE:
        if row.dtypes != ("f32", "f64"):
            assert (row.family, row.op, row.algo) == ("clouds", "raster", "chunked") and row.dtypes == ("f32",)
            q = dpr_amd.workspace_bytes_clouds("raster", row.grid, row.P, row.B, row.n_in, dtype=torch.float64,
                                               algo="chunked")
            assert q == 0
