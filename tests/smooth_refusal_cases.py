"""The refusal table of the smooth op families: every entry point, workspace query and AUTO resolver of the nine
families behind dpr_api_smooth.hip and dpr_api_smooth_bodies.hip, in f32 and f64, called once per way of spoiling one
argument of a valid call.  tests/golden/smooth_refusals.json holds, for every case, the status (or the value of a
query or resolver) and `says`, a short substring of the message that names the offending argument; it was recorded
from the library before the host checks of these families were folded into dpr_host_smooth.h, and
tests/test_smooth_refusals.py holds the library to it.

Every case ends in the host checks: the data pointers are dummies (256, misaligned: 258) and no device is needed.

    python tests/smooth_refusal_cases.py          # re-record the table from the library that dpr_amd loads
"""
import ctypes
import json
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smooth_refusals.json")
SIZE_MAX = ctypes.c_size_t(-1).value
RASTER, PULLBACK, RESIDUAL = 0, 1, 2
ATOMIC, TILED, CHUNKED, ORDERED = 1, 2, 3, 4
KEEP, REUSE = 1, 2
MPG2 = 2 << 8  # DPR_FLAG_MAX_POSE_GROUP(2)
DUMMY, ODD = 256, 258

SPLAT_FWD = ["out", "points", "rot", "trans", "bg", "ow", "pw"]
SPLAT_BWD = ["ds_dout", "points", "rot", "trans", "ow", "pw", "ds_dpoints", "ds_drot", "ds_dtrans", "ds_dbg", "ds_dow",
             "ds_dpw"]
SAMPLE_FWD = ["values", "image", "points", "rot", "trans"]
SAMPLE_BWD = ["ds_dvalues", "image", "points", "rot", "trans", "ds_dimage", "ds_dpoints", "ds_drot", "ds_dtrans"]
JVP_FWD = ["out_dot", "points", "rot", "trans", "ow", "pw", "points_dot", "rot_dot", "trans_dot", "bg_dot", "ow_dot",
           "pw_dot"]
# what the message says of a required pointer that is NULL
NULL_SAYS = {"out": "out is NULL", "points": "points is NULL", "body": "body is NULL", "rot": "rotation/translation",
             "trans": "rotation/translation", "pw": "point_weight is NULL", "ds_dout": "ds_dout is NULL",
             "ds_drot": "per-pose output", "ds_dtrans": "per-pose output", "ds_dbg": "per-pose output",
             "ds_dow": "per-pose output", "ds_dpoints": "ds_dpoints/ds_dpoint_weight",
             "ds_dpw": "ds_dpoints/ds_dpoint_weight", "values": "values is NULL", "image": "image is NULL",
             "ds_dvalues": "ds_dvalues is NULL", "out_dot": "out_dot is NULL"}
REQUIRED = {"fwd": {"splat": ["out", "points", "rot", "trans"], "sample": SAMPLE_FWD,
                    "jvp": ["out_dot", "points", "rot", "trans"]},
            "bwd": {"splat": ["ds_dout", "points", "rot", "trans", "ds_dpoints", "ds_drot", "ds_dtrans", "ds_dbg",
                              "ds_dow", "ds_dpw"],
                    "sample": ["ds_dvalues", "image", "points", "rot", "trans"]}}
POINTERS = {("fwd", "splat"): SPLAT_FWD, ("bwd", "splat"): SPLAT_BWD, ("fwd", "sample"): SAMPLE_FWD,
            ("bwd", "sample"): SAMPLE_BWD, ("fwd", "jvp"): JVP_FWD}

BIG = (1024, 1024, 1024)  # 2^30 cells
P_BLOCKS = ("P blocks", dict(P=1 << 40))
P_B = ("P * B", dict(P=1 << 33, B=1 << 30))
G_B = ("G * B", dict(B=1 << 51))
B_ALONE = ("B", dict(B=1 << 48))

# name: the stem of the C names; shape: the argument lists; extents: the arguments after B with their valid values;
# tiled: the op that may run DPR_ALGO_TILED; mpg: the (kind, op) whose ATOMIC call refuses DPR_FLAG_MAX_POSE_GROUP;
# sizes: the 64-bit size bounds, each with the arguments that pass it alone (rigid bodies: with K = 1)
Family = namedtuple("Family", "name fwd bwd shape extents residual tiled body needs_pw mpg sizes")
FAMILIES = [
    Family("smooth", "dpr_raster_smooth_ex", "dpr_raster_pullback_smooth_ex", "splat", {}, True, RASTER, False, False,
           (), [P_BLOCKS]),
    Family("sample_smooth", "dpr_sample_smooth_ex", "dpr_sample_smooth_pullback_ex", "sample", {}, False, PULLBACK,
           False, False, (), [P_BLOCKS, P_B, G_B, B_ALONE]),
    Family("smooth_jvp", "dpr_raster_smooth_jvp_ex", None, "jvp", {"V": 3}, False, None, False, False, (),
           [P_BLOCKS, P_B, G_B, B_ALONE, ("G * V * B", dict(grid=BIG, V=16, B=1 << 29))]),
    Family("smooth_clouds", "dpr_raster_smooth_clouds_ex", "dpr_raster_pullback_smooth_clouds_ex", "splat", {}, True,
           RASTER, False, False, (), [P_BLOCKS, ("B * P * n_in", dict(P=1 << 33, B=1 << 30)), G_B]),
    Family("smooth_channels", "dpr_raster_smooth_channels_ex", "dpr_raster_pullback_smooth_channels_ex", "splat",
           {"C": 3}, True, RASTER, False, True, (), [P_BLOCKS, ("G * C * B", dict(grid=BIG, C=16, B=1 << 29))]),
    Family("sample_smooth_channels", "dpr_sample_smooth_channels_ex", "dpr_sample_smooth_channels_pullback_ex",
           "sample", {"C": 3}, False, PULLBACK, False, False, (),
           [P_BLOCKS, P_B, G_B, B_ALONE, ("P * C * B", dict(P=1 << 33, B=1 << 26, C=16)),
            ("G * C * B", dict(grid=BIG, C=16, B=1 << 29))]),
    Family("smooth_bodies", "dpr_raster_smooth_bodies_ex", "dpr_raster_pullback_smooth_bodies_ex", "splat", {"K": 3},
           True, RASTER, True, False, (("bwd", PULLBACK),), [P_BLOCKS]),
    Family("smooth_bodies_jvp", "dpr_raster_smooth_bodies_jvp_ex", None, "jvp", {"K": 3, "V": 3}, False, None, True,
           False, (), [P_BLOCKS, ("P * B", dict(P=1 << 33, B=1 << 30, K=1)),
                       ("G * V * B", dict(grid=BIG, V=16, B=1 << 29, K=1))]),
    Family("sample_smooth_bodies", "dpr_sample_smooth_bodies_ex", "dpr_sample_smooth_bodies_pullback_ex", "sample",
           {"K": 3}, False, PULLBACK, True, False, (("fwd", RASTER), ("bwd", PULLBACK)),
           [P_BLOCKS, ("P * B", dict(P=1 << 33, B=1 << 30, K=1))]),
]
BASE = dict(algo=ATOMIC, flags=0, n_in=3, n_out=3, grid=(16, 16, 16), P=10, B=2, ws=None, wsb=0)


def _pointers(fam, kind):
    names = list(POINTERS[(kind, fam.shape)])
    if fam.body:
        names.insert(names.index("points") + 1, "body")
    return names


def call(L, fam, kind, suf, over):
    """One call of (family, kind) with `over` laid over the valid call; kind is fwd, bwd, query or resolve, and `op` in
    `over` picks the op of a query or resolver.  Returns (value, message)."""
    a = dict(BASE, **fam.extents)
    a.update(over)
    grid = np.asarray(a["grid"], dtype=np.int64) if a["grid"] is not None else None
    gp = grid.ctypes.data_as(ctypes.c_void_p) if grid is not None else None
    shape = [a["n_in"], a["n_out"], gp, a["P"], a["B"]] + [a[e] for e in fam.extents]
    op = [] if fam.shape == "jvp" else [a.get("op", RASTER)]
    if kind == "resolve":
        v = getattr(L, "dpr_resolve_algo_" + fam.name)(*op, *shape)
    elif kind == "query":
        v = getattr(L, f"dpr_workspace_bytes_{fam.name}_ex_{suf}")(*op, a["algo"], a["flags"], *shape)
    else:
        ptrs = [ctypes.c_void_p(a.get(n, DUMMY)) for n in _pointers(fam, kind)]
        ws = ctypes.c_void_p(a["ws"]) if a["ws"] is not None else None
        f = getattr(L, f"{fam.fwd if kind == 'fwd' else fam.bwd}_{suf}")
        v = f(None, a["algo"], a["flags"], *shape, *ptrs, ws, a["wsb"])
    return v, L.dpr_last_error().decode("utf-8", "replace")


def spoils(L, fam, kind, suf, op):
    """(label, overrides, says) of every case of one function; says is None where the call is accepted.  `op`: the op
    of the entry point, or the one a query or resolver is asked about (None: the family has one op)."""
    entry = kind in ("fwd", "bwd")
    takes_algo = kind != "resolve"
    out = [("pair (2,3)", dict(n_in=2, n_out=3, grid=(16, 16, 16)), "(2,2), (3,3), (3,2)"),
           ("n_in = 5", dict(n_in=5), "(2,2), (3,3), (3,2)"),
           ("grid NULL", dict(grid=None), "grid is NULL"),
           ("P = -1", dict(P=-1), "negative"),
           ("B = -1", dict(B=-1), "negative")]
    if not entry and op is not None:
        out.append(("op = 9", dict(op=9), "op 9"))
        out.append(("residual op", dict(op=RESIDUAL), "residual pullback" if fam.residual else "op 2"))
    if takes_algo:
        out.append(("KEEP", dict(flags=KEEP), "binning"))
        out.append(("REUSE", dict(flags=REUSE), "binning"))
        for algo in (CHUNKED, ORDERED, 9):
            out.append((f"algo = {algo}", dict(algo=algo), f"algorithm {algo}"))
        if op is not None and op != fam.tiled:
            out.append(("TILED", dict(algo=TILED), "ATOMIC only"))
        if any(o == op and (not entry or k == kind) for k, o in fam.mpg):
            out.append(("MAX_POSE_GROUP", dict(flags=MPG2), "DPR_FLAG_MAX_POSE_GROUP"))
    if "C" in fam.extents:
        out += [("C = 0", dict(C=0), "C = 0"), ("C = 17", dict(C=17), "C = 17")]
    if "K" in fam.extents:
        out += [("K = 0", dict(K=0), "at least one body"),
                ("B * K = 2^31", dict(B=1 << 16, K=1 << 15), "exceed 2^31 - 1")]
    if "V" in fam.extents:
        out += [("V = 0", dict(V=0), "tangents"), ("V = 17", dict(V=17), "tangents")]
    for label, over in fam.sizes:
        out.append((label + " too large", over, "too large"))
    tiled_op = op is None or op == fam.tiled
    if takes_algo and tiled_op:
        out.append(("P = 2^32 - 1, TILED", dict(algo=TILED, P=(1 << 32) - 1), "2^32 - 2"))
    if entry:
        names = _pointers(fam, kind)
        required = REQUIRED[kind][fam.shape] + (["body"] if fam.body else []) + (["pw"] if fam.needs_pw else [])
        for n in names:
            if n in required:
                out.append((n + " NULL", {n: None}, NULL_SAYS[n]))
            out.append((n + " misaligned", {n: ODD}, "aligned"))
        if kind == "bwd" and fam.shape == "sample":
            out.append(("every output NULL", dict(ds_dimage=None, ds_dpoints=None, ds_drot=None, ds_dtrans=None),
                        "every output is NULL"))
        if tiled_op:
            q = dict(op=op) if op is not None else {}
            need, _ = call(L, fam, "query", suf, dict(q, algo=TILED))
            assert need not in (0, SIZE_MAX), (fam.name, kind, need)
            out += [("TILED, workspace NULL", dict(algo=TILED), "workspace"),
                    ("TILED, workspace short", dict(algo=TILED, ws=DUMMY, wsb=need - 1), "workspace"),
                    ("TILED, workspace misaligned", dict(algo=TILED, ws=ODD, wsb=need), "256-byte aligned")]
        out.append(("no poses, no points", dict(B=0, P=0), None))
    if op is not None:
        out = [(label, dict(dict(op=op), **over), says) for label, over, says in out]
    return out


def functions():
    """(id, family, kind, suf, op) of every function of the table; queries and resolvers once per op they take."""
    for fam in FAMILIES:
        ops = [None] if fam.shape == "jvp" else [RASTER, PULLBACK]
        for op in ops:
            tag = "" if op is None else (" of the forward" if op == RASTER else " of the pullback")
            yield f"{fam.name}: resolver{tag}", fam, "resolve", None, op
        for suf in ("f32", "f64"):
            for op in ops:
                tag = "" if op is None else (" of the forward" if op == RASTER else " of the pullback")
                yield f"{fam.name}: query{tag}, {suf}", fam, "query", suf, op
            yield f"{fam.name}: forward, {suf}", fam, "fwd", suf, None if fam.shape == "jvp" else RASTER
            if fam.bwd:
                yield f"{fam.name}: pullback, {suf}", fam, "bwd", suf, PULLBACK


def record(L):
    """{function: {case: [value, says]}} from the library L; checks that every refusal says what the case expects."""
    table = {}
    for fid, fam, kind, suf, op in functions():
        rows = table[fid] = {}
        for label, over, says in spoils(L, fam, kind, suf, op):
            v, msg = call(L, fam, kind, suf, over)
            v = -1 if v == SIZE_MAX else v
            if says is None:
                assert v == 0, (fid, label, v, msg)
            elif v >= 0:  # a query or resolver that does not look at this argument: its answer is the record
                assert kind in ("query", "resolve"), (fid, label, v)
                says = None
            else:
                assert says in msg, (fid, label, says, msg)
            rows[label] = [v, says]
    return table


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import dpr_amd

    table = record(dpr_amd.lib())
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(r) for r in table.values())} cases of {len(table)} functions -> {GOLDEN}")
