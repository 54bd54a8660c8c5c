"""The workspace sizes of the smooth families, pinned value by value (no GPU needed).

One plan (smooth_plan of dpr_smooth.hip) lays out the workspace of every tiled smooth launcher, for a pose at a
time or for a group of poses, and the seven workspace queries answer from it.  tests/golden/smooth_workspace_bytes.json
holds what `dpr_workspace_bytes_{smooth, sample_smooth, smooth_jvp, smooth_clouds, smooth_channels, smooth_bodies,
smooth_bodies_jvp}_ex_*` answer for DPR_ALGO_TILED and DPR_ALGO_AUTO over a sweep that reaches every term of the
plan: point counts around a block, around the 2^24 of the group rule and at the 32-bit end; pose counts and
DPR_FLAG_MAX_POSE_GROUP values that leave a shorter last group (B % bg != 0, the `last` term of smooth_plan); grids on
and just past a tile edge; the refusals.  Any change of the plan or of the group rule shows here first.

The record has two parts, because one term of the plan is not the library's own: the temporary storage of the radix
sort is what rocPRIM's size query answers, and that query answers 0 where no HIP device is present.  "layout" holds
the answers of a machine without a device -- everything but that term -- and "sort_gfx950" what an MI355X adds to each
of them.  The test expects layout alone, or the sum, by what `dpr_sort_points_workspace_bytes` shows of the machine it
runs on; it passes in both places.

The refusal "too many tiles for a 32-bit key" has two arms.  P > 2^32 - 2 is in the sweep (P = 2^32 - 1).  The tile
count itself cannot be reached through a query: check_common holds a grid to 2^31 - 1 cells, far fewer tiles than
2^31 - 1.  The refused grid of each dimension is therefore one that check_common turns away.

    python -m tests.test_smooth_workspace_golden [FILE]   # records this machine's part from the library as built
                                                          # ("sort_gfx950" needs the "layout" part in FILE already)
"""
import ctypes
import itertools
import json
import os
import sys

import dpr_amd
from dpr_amd import _lib
from tests.conftest import ROOT
from tests.test_tiled_workspace_golden import REFUSED, SUFFIXES, _pack, _unpack

GOLDEN = os.path.join(ROOT, "tests", "golden", "smooth_workspace_bytes.json")

# tiles are 64 x 16 and 16 x 8 x 8: a grid of one tile and one a cell past it on every axis, the workload grids, and
# a grid the checks refuse
GRIDS_2D = ((64, 16), (65, 17), (128, 128), (4096, 4096), (65536, 32768))
GRIDS_3D = ((16, 8, 8), (17, 9, 9), (128,) * 3, (256,) * 3, (2048,) * 3)
SHAPES = [(n_in, n_out, g) for n_in, n_out in ((2, 2), (3, 3), (3, 2)) for g in (GRIDS_3D if n_out == 3 else GRIDS_2D)]
POINTS = (0, 1, 255, 256, 257, 1000, 10**5, 2**24, 2**24 + 1, 2**32 - 2, 2**32 - 1)
POSES = (1, 2, 3, 5, 16, 64)
GROUPS = (0, 1, 2, 3, 7)  # DPR_FLAG_MAX_POSE_GROUP, for the families that bin groups of poses
OPS = (_lib.OP_RASTER, _lib.OP_PULLBACK)
ALGOS = (_lib.ALGO_TILED, _lib.ALGO_AUTO)
CHANNELS = 3  # weights per point, tangents
BODIES = 2

# query -> (has an op argument, honours DPR_FLAG_MAX_POSE_GROUP, trailing arguments)
QUERIES = {
    "smooth": (True, False, ()),
    "sample_smooth": (True, False, ()),
    "smooth_jvp": (False, False, (CHANNELS,)),
    "smooth_clouds": (True, True, ()),
    "smooth_channels": (True, False, (CHANNELS,)),
    "smooth_bodies": (True, True, (BODIES,)),
    "smooth_bodies_jvp": (False, True, (BODIES, CHANNELS)),
}


def _sweeps():
    """{query: [(label of the case, its answer), ...]} in sweep order, from the library as built."""
    L = dpr_amd.lib()
    grid = lambda g: (ctypes.c_int64 * 3)(*g, *([1] * (3 - len(g))))
    out = {}
    for query, (has_op, grouped, tail) in QUERIES.items():
        cases = out[query] = []
        fs = [(suf, getattr(L, f"dpr_workspace_bytes_{query}_ex_{suf}")) for suf in SUFFIXES]
        # (the element type innermost, then B: neighbours in the record are mostly equal, which is what deflate likes)
        for (n_in, n_out, g), algo, op, P in itertools.product(SHAPES, ALGOS, OPS if has_op else (None,), POINTS):
            gp = grid(g)
            for group, B, (suf, f) in itertools.product(GROUPS if grouped else (0,), POSES, fs):
                flags = _lib.flag_max_pose_group(group) if group else 0
                head = (algo, flags) if op is None else (op, algo, flags)
                n = f(*head, n_in, n_out, gp, P, B, *tail)
                cases.append((f"{suf} {n_in}->{n_out} {g} P={P} B={B} algo={algo} op={op} group={group}", n))
    return out


def _rocprim_sizes_the_sort():
    """Whether the sort's temporary storage is counted on this machine: dpr_sort_points_workspace_bytes(P) is three
    arrays of P 32-bit words, each rounded up to 256 bytes, plus that storage."""
    L = dpr_amd.lib()
    L.dpr_sort_points_workspace_bytes.restype = ctypes.c_size_t
    L.dpr_sort_points_workspace_bytes.argtypes = [ctypes.c_int64]
    P = 2**21
    return L.dpr_sort_points_workspace_bytes(P) > 3 * 4 * P


def _add(layout, sort):
    return [a if a == REFUSED else a + b for a, b in zip(layout, sort)]


def test_smooth_workspace_sizes_match_the_record():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _sweeps()
    assert sorted(want) == ["layout", "sort_gfx950"]
    assert sorted(want["layout"]) == sorted(want["sort_gfx950"]) == sorted(got)
    with_sort = _rocprim_sizes_the_sort()
    for query, cases in got.items():
        expect = _unpack(want["layout"][query])
        if with_sort:
            expect = _add(expect, _unpack(want["sort_gfx950"][query]))
        assert len(expect) == len(cases), f"{query}: the record holds {len(expect)} answers, the sweep {len(cases)}"
        wrong = [f"{label}: {n} bytes, recorded {e}" for (label, n), e in zip(cases, expect) if n != e]
        assert not wrong, f"{query}: {len(wrong)} of {len(cases)} answers differ, first:\n" + "\n".join(wrong[:10])
        assert REFUSED in expect and any(e not in (REFUSED, 0) for e in expect)  # refusals are part of the record


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    got = {q: [n for _, n in cases] for q, cases in _sweeps().items()}
    if _rocprim_sizes_the_sort():
        with open(path) as f:
            record = json.load(f)
        record["sort_gfx950"] = {}
        for q, answers in got.items():
            layout = _unpack(record["layout"][q])
            assert all((a == REFUSED) == (b == REFUSED) and a >= b for a, b in zip(answers, layout)), q
            record["sort_gfx950"][q] = _pack([0 if a == REFUSED else a - b for a, b in zip(answers, layout)])
    else:
        record = {"layout": {q: _pack(answers) for q, answers in got.items()}, "sort_gfx950": {}}
    with open(path, "w") as f:
        json.dump(record, f, indent=0)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
