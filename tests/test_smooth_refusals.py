"""The smooth op families against their recorded refusal table (tests/smooth_refusal_cases.py,
tests/golden/smooth_refusals.json): every entry point, workspace query and AUTO resolver, f32 and f64, with one
argument of a valid call spoiled.  The status -- or the value of a query or resolver -- is the recorded one, and the
message names the offending thing.  With two arguments spoiled the library may refuse either, in the one order that
csrc/dpr_host_smooth.h documents; an unsupported (n_in, n_out) wins over everything.  No GPU needed: every call ends
in the host checks."""
import itertools
import json

import pytest

import dpr_amd
from dpr_amd import _lib
from tests import smooth_refusal_cases as cases

TABLE = json.load(open(cases.GOLDEN))
FUNCTIONS = list(cases.functions())


def _value(v):
    return -1 if v == cases.SIZE_MAX else v


def test_the_table_covers_every_function_of_the_nine_families():
    assert sorted(TABLE) == sorted(f[0] for f in FUNCTIONS)
    assert len(FUNCTIONS) == 80
    L = dpr_amd.lib()
    for fid, fam, kind, suf, op in FUNCTIONS:
        assert sorted(TABLE[fid]) == sorted(label for label, _, _ in cases.spoils(L, fam, kind, suf, op)), fid


@pytest.mark.parametrize("fid,fam,kind,suf,op", FUNCTIONS, ids=[f[0] for f in FUNCTIONS])
def test_one_spoiled_argument(fid, fam, kind, suf, op):
    L = dpr_amd.lib()
    for label, over, _ in cases.spoils(L, fam, kind, suf, op):
        want, says = TABLE[fid][label]
        v, msg = cases.call(L, fam, kind, suf, over)
        assert _value(v) == want, (label, v, want, msg)
        if says is not None:
            assert says in msg, (label, says, msg)


@pytest.mark.parametrize("fid,fam,kind,suf,op", FUNCTIONS, ids=[f[0] for f in FUNCTIONS])
def test_two_spoiled_arguments(fid, fam, kind, suf, op):
    """Pairs of refusals with different statuses that spoil different arguments: one of the two statuses comes back,
    DPR_ERR_UNSUPPORTED_DIMS where the pair (n_in, n_out) is one of the faults."""
    L = dpr_amd.lib()
    refused = [(label, over) for label, over, _ in cases.spoils(L, fam, kind, suf, op) if TABLE[fid][label][0] < 0]
    assert len(refused) >= 7
    pairs = 0
    for (la, oa), (lb, ob) in itertools.combinations(refused, 2):
        sa, sb = TABLE[fid][la][0], TABLE[fid][lb][0]
        # (every case carries the op of its function: only "op = 9" and "residual op" spoil it)
        if (kind != "query" and sa == sb) or any(k != "op" and oa[k] != ob[k] for k in oa.keys() & ob.keys()):
            continue
        # (DPR_ALGO_TILED at the P of a size bound is a third fault: P > 2^32 - 2)
        if any(x.get("algo") == cases.TILED and "P" in y and y["P"] > 1 << 32 for x, y in ((oa, ob), (ob, oa))):
            continue
        both = dict(oa, **ob)
        if op is not None and oa["op"] != op:
            both["op"] = oa["op"]
        v, msg = cases.call(L, fam, kind, suf, both)
        if kind != "query":
            want = {sa, sb}
            if _lib.ERR_UNSUPPORTED_DIMS in want:
                want = {_lib.ERR_UNSUPPORTED_DIMS}
            assert v in want, (la, lb, v, msg)
        else:
            assert v == cases.SIZE_MAX, (la, lb, v, msg)
        pairs += 1
    assert pairs > 0


def test_the_largest_P_is_too_large():
    """check_point_blocks counts the blocks of P = 2^63 - 1 without overflow: wherever a function refuses the P of the
    table's block bound, it refuses the largest P alike."""
    L = dpr_amd.lib()
    n = 0
    for fid, fam, kind, suf, op in FUNCTIONS:
        want, says = TABLE[fid]["P blocks too large"]
        if want >= 0:
            continue
        over = next(o for label, o, _ in cases.spoils(L, fam, kind, suf, op) if label == "P blocks too large")
        v, msg = cases.call(L, fam, kind, suf, dict(over, P=(1 << 63) - 1))
        assert _value(v) == want and says in msg, (fid, v, msg)
        n += 1
    assert n == 72
