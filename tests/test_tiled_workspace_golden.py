"""The workspace sizes of DPR_ALGO_TILED, pinned value by value (no GPU needed).

The layout of the tiled workspace is a contract between calls: a KEEP_BINNING forward, the REUSE_BINNING
pullback that consumes its binning and the workspace query each compute the plan on their own, and a
workspace sized by one build of the library has to serve the next.  tests/golden/tiled_workspace_bytes.json
holds what `dpr_workspace_bytes_ex_*`, `dpr_workspace_bytes_channels_ex_*` and `dpr_workspace_bytes_jvp_ex_*`
answer for DPR_ALGO_TILED over a sweep that reaches every branch of the plan (pose groups, local binning, the
cell sort inside the call, kept batches, slabs, the refusals); any change of the plan shows here first.

    python -m tests.test_tiled_workspace_golden     # records the file from the library as built
"""
import base64
import ctypes
import itertools
import json
import os
import struct
import zlib

import dpr_amd
from dpr_amd import _lib
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "tiled_workspace_bytes.json")

SUFFIXES = ("f32", "f64")
# (n_in, n_out) and the grids of that n_out; 768^3 and 1024^3 are cut into slabs
GRIDS_2D = ((128, 128), (512, 512), (4096, 4096))
GRIDS_3D = ((64,) * 3, (128,) * 3, (256,) * 3, (768,) * 3, (1024,) * 3)
SHAPES = [(n_in, n_out, g) for n_in, n_out in ((2, 2), (3, 3), (3, 2)) for g in (GRIDS_3D if n_out == 3 else GRIDS_2D)]
POINTS = (0, 1, 1_000, 199_999, 200_000, 10**6, 10**7, 2**27 + 1, 2**32)
POSES = (1, 2, 3, 4, 16, 64)
FLAGS = (0, _lib.FLAG_KEEP_BINNING, _lib.FLAG_REUSE_BINNING, _lib.FLAG_COHERENT_POINTS,
         _lib.FLAG_COHERENT_POINTS | _lib.FLAG_KEEP_BINNING, _lib.flag_max_pose_group(1), _lib.flag_max_pose_group(4))
OPS = (_lib.OP_RASTER, _lib.OP_PULLBACK)
CHANNELS = (1, 3, 16)
REFUSED = ctypes.c_size_t(-1).value


def _sweeps():
    """{query: [(label of the case, its answer), ...]} in sweep order, from the library as built."""
    L = dpr_amd.lib()
    grid = lambda g: (ctypes.c_int64 * 3)(*g, *([1] * (3 - len(g))))
    out = {"workspace": [], "channels": [], "jvp": []}
    for suf, (n_in, n_out, g), P in itertools.product(SUFFIXES, SHAPES, POINTS):
        gp = grid(g)
        for B, flags, op in itertools.product(POSES, FLAGS, OPS):
            n = getattr(L, f"dpr_workspace_bytes_ex_{suf}")(op, _lib.ALGO_TILED, flags, n_in, n_out, gp, P, B)
            out["workspace"].append((f"{suf} {n_in}->{n_out} {g} P={P} B={B} flags={flags:#x} op={op}", n))
        for B, C in itertools.product(POSES, CHANNELS):
            n = getattr(L, f"dpr_workspace_bytes_channels_ex_{suf}")(_lib.OP_RASTER, _lib.ALGO_TILED, 0, n_in, n_out,
                                                                    gp, P, B, C)
            out["channels"].append((f"{suf} {n_in}->{n_out} {g} P={P} B={B} C={C}", n))
        for B in POSES:
            n = getattr(L, f"dpr_workspace_bytes_jvp_ex_{suf}")(_lib.ALGO_TILED, 0, n_in, n_out, gp, P, B, 1)
            out["jvp"].append((f"{suf} {n_in}->{n_out} {g} P={P} B={B}", n))
    return out


def _pack(values):
    """A list of answers as text: the values as little-endian int64 ((size_t)-1 is -1), deflated, base64 -- the
    sweep has 21 384 cases, written out as numbers they would be the largest file under tests/golden."""
    raw = struct.pack(f"<{len(values)}q", *(-1 if v == REFUSED else v for v in values))
    return base64.b64encode(zlib.compress(raw, 9)).decode("ascii")


def _unpack(text):
    raw = zlib.decompress(base64.b64decode(text))
    return [REFUSED if v == -1 else v for v in struct.unpack(f"<{len(raw) // 8}q", raw)]


def test_tiled_workspace_sizes_match_the_record():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _sweeps()
    assert sorted(want) == sorted(got)
    for query, cases in got.items():
        expect = _unpack(want[query])
        assert len(expect) == len(cases), f"{query}: the record holds {len(expect)} answers, the sweep {len(cases)}"
        wrong = [f"{label}: {n} bytes, recorded {e}" for (label, n), e in zip(cases, expect) if n != e]
        assert not wrong, f"{query}: {len(wrong)} of {len(cases)} answers differ, first:\n" + "\n".join(wrong[:10])
        assert REFUSED in expect and any(e != REFUSED for e in expect)  # refusals are part of the record


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({q: _pack([n for _, n in cases]) for q, cases in _sweeps().items()}, f, indent=0)
        f.write("\n")
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
