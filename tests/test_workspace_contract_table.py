"""(CPU)  The table of tests/workspace_cases.py is complete: every public `workspace_bytes*` query, every algorithm it
accepts and every flag set that moves its layout, asked at the table's own shapes, either needs no workspace or has
a row -- so a later op family, algorithm or layout flag cannot slip past tests/test_workspace_contract_gpu.py.

A row is looked up by (family, op, algorithm, flag set, element type) and, without flags, by the dimension of the
grid as well (2-D and 3-D grids run different kernels everywhere; the flag sets of DPR_ALGO_TILED and of the smooth
clouds are held on one grid each, DPR_FLAG_COHERENT_POINTS on DPR_ALGO_CHUNKED on both).
What the walk leaves out, and why:
  * DPR_ALGO_AUTO: it resolves to one of the named algorithms, whose rows stand for it;
  * the residual pullback with DPR_FLAG_MAX_POSE_GROUP: raster_residual_pullback_ has no such argument, the C entry
    point runs pullback_tiled with the flags of the plain pullback's rows;
  * the forwards of 3-D DPR_ALGO_CHUNKED that sort inside the call (B >= 8 and P >= 2e5, csrc/dpr_api.hip): two
    hundred thousand points are no shape of this table; their layout is the Hilbert sort's (Q1 in DESIGN.md 4.18)
    in front of the owner or chunk-list layout, and they are audited there.
"""
import functools
import os
import re

import pytest

import dpr_amd
from dpr_amd import _lib
from tests.workspace_cases import FLAGS, QUERIES, TABLE, TDT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (family, op, flag set): no Python argument carries the flag to this op
NO_ARGUMENT = {("core", "residual_pullback", f) for f in ("mpg1", "mpg2", "local")}


def key(family, op, algo, flags, dt, grid):
    one_grid = flags and algo != "chunked"  # (DPR_ALGO_CHUNKED is two algorithms: its flag set is held on both)
    return (family, op, algo, flags, dt, None if one_grid else len(grid))


def covered(table):
    keys = set()
    for r in table:
        for op in (("raster", "pullback", "residual_pullback") if r.op == "pair" else (r.op,)):
            keys.update(key(r.family, op, r.algo, r.flags, dt, r.grid) for dt in r.dtypes)
    return keys


@functools.lru_cache(maxsize=None)
def walk():
    """Every (family, op, algo, flags, dt, grid dimension) whose query is non-zero at a shape of the table."""
    shapes = sorted({(r.n_in, r.grid, r.P, r.B) for r in TABLE})
    found = {}
    for name, (family, ops, flag_sets, query) in QUERIES.items():
        for algo in (a for a in _lib.ALGOS if a != "auto"):
            for flags in ("",) + tuple(f for f in flag_sets.get(algo, ()) if f):
                for op in ops:
                    if (family, op, flags) in NO_ARGUMENT:
                        continue
                    for dt, tdt in TDT.items():
                        for n_in, grid, P, B in shapes:
                            try:
                                need = query(op, algo, flags, n_in, grid, P, B, tdt)
                            except dpr_amd.DprError:
                                continue  # the family does not run this algorithm / op / shape
                            if need:
                                found.setdefault(key(family, op, algo, flags, dt, grid), (name, n_in, grid, P, B, need))
    return found


def missing(table):
    have = covered(table)
    return {k: v for k, v in walk().items() if k not in have}


def test_every_public_workspace_query_is_walked():
    public = sorted(n for n in dir(dpr_amd) if n.startswith("workspace_bytes"))
    assert public == sorted(QUERIES), "a workspace_bytes* function without an entry in tests/workspace_cases.py"
    for name in QUERIES:
        assert name in dpr_amd.__all__
    assert set(FLAGS) >= {f for _fam, _ops, sets, _q in QUERIES.values() for fs in sets.values() for f in fs}


def test_every_non_zero_query_has_a_row():
    lacking = missing(TABLE)
    assert not lacking, "\n".join(f"{k}: {v[0]}{v[1:5]} needs {v[5]} bytes and has no row" for k, v in lacking.items())
    # and the other way round: a row whose query is zero or refused tests nothing
    found = walk()
    for k in covered(TABLE):
        assert k in found, f"row {k}: the query is zero or refused at every shape of the table"


def test_the_walk_notices_a_missing_row():
    """Without any one row the walk fails -- except where two rows share a key, which one query serves at two
    shapes: the owner tiles and the chunk lists of the 3-D DPR_ALGO_CHUNKED forward (B = 3 and B = 4), and the
    per-pose cloud forward on DPR_ALGO_CHUNKED with two slices and with one (3001 and 2001 points)."""
    shared = []
    for i, row in enumerate(TABLE):
        rest = TABLE[:i] + TABLE[i + 1:]
        if not missing(rest):
            shared.append(row)
    assert {(r.family, r.op, r.algo, r.flags, len(r.grid)) for r in shared} == {
        ("core", "raster", "chunked", "", 3), ("clouds", "raster", "chunked", "", 2), ("clouds", "raster", "chunked", "", 3)}
    assert sorted((r.family, r.P, r.B) for r in shared) == [
        ("clouds", 2001, 3), ("clouds", 2001, 3), ("clouds", 3001, 3), ("clouds", 3001, 3), ("core", 3001, 3),
        ("core", 3001, 4)]


def test_rows_point_to_the_audit_in_design_md():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.18"):]
    ids = set(re.findall(r"^\| ([A-Z]\d) \|", section, re.M))
    for r in TABLE:
        assert r.audit in ids, f"{r}: no line {r.audit} in the audit table of DESIGN.md 4.18"
    # a row is spared the all-ones pattern only with a reason in that table
    for r in TABLE:
        if not r.poison:
            assert re.search(rf"^\| {r.audit} \|.*all-ones pattern not run", section, re.M), r


@pytest.mark.parametrize("path", ["include/dpr.h", "DESIGN.md", "INTEGRATION.md"])
def test_the_contract_is_written_down(path):
    text = " ".join(open(os.path.join(ROOT, path)).read().replace("*", " ").split())
    for sentence in ("The initial contents of the workspace do not matter",
                     "writes only inside [workspace, workspace + workspace_bytes)",
                     "What a call leaves in the workspace is unspecified",
                     "only enqueues on `stream`",
                     "captured into a HIP graph"):
        assert sentence in text, f"{path}: {sentence!r}"
