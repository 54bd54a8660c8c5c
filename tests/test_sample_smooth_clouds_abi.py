"""Host-side checks of the C ABI of smooth sampling at per-pose clouds (include/dpr.h, SMOOTH SAMPLING, PER-POSE
CLOUDS): prototypes and exports, the AUTO rule against dpr_resolve_algo_smooth_clouds over the shapes of
tests/golden/smooth_clouds_auto.json, workspace sizes against the splat's, every refusal (the cases of
tests/smooth_refusal_cases.py for this family) and the order of refusals of csrc/dpr_host_smooth.h.  No GPU needed:
every refused call returns before anything is launched, with dummy pointers that are never dereferenced."""
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
from tests import smooth_refusal_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dpr_resolve_algo_sample_smooth_clouds", "dpr_workspace_bytes_sample_smooth_clouds_ex_f32",
       "dpr_workspace_bytes_sample_smooth_clouds_ex_f64", "dpr_sample_smooth_clouds_ex_f32",
       "dpr_sample_smooth_clouds_ex_f64", "dpr_sample_smooth_clouds_pullback_ex_f32",
       "dpr_sample_smooth_clouds_pullback_ex_f64"]
SIZE_MAX = ctypes.c_size_t(-1).value
PAIRS = [(2, 2), (3, 3), (3, 2)]
RASTER, PULLBACK = _lib.OP_RASTER, _lib.OP_PULLBACK
GOLDEN_AUTO = os.path.join(ROOT, "tests", "golden", "smooth_clouds_auto.json")

# the family in the terms of tests/smooth_refusal_cases.py: the sampling argument lists, DPR_ALGO_TILED on the
# pullback, DPR_FLAG_MAX_POSE_GROUP never refused; the size bounds of the smooth cloud splat and smooth sampling's P * B
FAMILY = cases.Family("sample_smooth_clouds", "dpr_sample_smooth_clouds_ex", "dpr_sample_smooth_clouds_pullback_ex",
                      "sample", {}, False, PULLBACK, False, False, (),
                      [cases.P_BLOCKS, ("B * P * n_in", dict(P=1 << 33, B=1 << 30)), cases.G_B, cases.P_B])
FUNCTIONS = [("resolver of the forward", "resolve", None, RASTER), ("resolver of the pullback", "resolve", None, PULLBACK)]
for _suf in ("f32", "f64"):
    FUNCTIONS += [(f"query of the forward, {_suf}", "query", _suf, RASTER),
                  (f"query of the pullback, {_suf}", "query", _suf, PULLBACK),
                  (f"forward, {_suf}", "fwd", _suf, RASTER), (f"pullback, {_suf}", "bwd", _suf, PULLBACK)]
# the status that goes with what a message says (the first match; "256-byte aligned" before "aligned")
STATUS = [("(2,2), (3,3), (3,2)", _lib.ERR_UNSUPPORTED_DIMS), ("binning", _lib.ERR_UNSUPPORTED_ALGO),
          ("algorithm ", _lib.ERR_UNSUPPORTED_ALGO), ("ATOMIC only", _lib.ERR_UNSUPPORTED_ALGO),
          ("2^32 - 2", _lib.ERR_UNSUPPORTED_ALGO), ("256-byte aligned", _lib.ERR_WORKSPACE),
          ("workspace", _lib.ERR_WORKSPACE)]


def _g(grid):
    a = np.asarray(grid, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _status(says):
    return next((s for text, s in STATUS if text in says), _lib.ERR_INVALID_ARG)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "dpr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = dpr_amd.lib()
    assert len(NEW) == 7
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    for name in ("sample_smooth_clouds", "sample_smooth_clouds_", "sample_smooth_clouds_pullback_",
                 "sample_smooth_clouds_ad", "resolve_algo_sample_smooth_clouds"):
        assert callable(getattr(dpr_amd, name)), name
        assert name in dpr_amd.__all__
    # the workspace query, with max_pose_group like the splat's: an attribute of the package and of its module, kept
    # off `__all__` (tests/workspace_cases.py walks the `workspace_bytes*` names there; this plan is the splat's)
    module = sys.modules[dpr_amd.sample_smooth_clouds.__module__]
    assert dpr_amd._pkg.workspace_bytes_sample_smooth_clouds is module.workspace_bytes_sample_smooth_clouds
    assert "workspace_bytes_sample_smooth_clouds" not in dpr_amd.__all__
    assert "SMOOTH SAMPLING, PER-POSE CLOUDS" in header


def test_prototypes_are_those_of_smooth_sampling():
    text = open(os.path.join(ROOT, "include", "dpr.h")).read()

    def proto(name):
        m = re.search(rf"\b{name}\s*\((.*?)\);", text, flags=re.S)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1))

    for name in ("dpr_resolve_algo_sample_smooth{}", "dpr_workspace_bytes_sample_smooth{}_ex_f32",
                 "dpr_workspace_bytes_sample_smooth{}_ex_f64", "dpr_sample_smooth{}_ex_f32",
                 "dpr_sample_smooth{}_ex_f64", "dpr_sample_smooth{}_pullback_ex_f32",
                 "dpr_sample_smooth{}_pullback_ex_f64"):
        assert proto(name.format("_clouds")) == proto(name.format("")), name


def test_auto_is_atomic_forward_and_the_smooth_cloud_forwards_choice_for_the_pullback():
    L = dpr_amd.lib()
    shapes = json.load(open(GOLDEN_AUTO))["shapes"]
    assert len(shapes) > 10
    seen = set()
    for s in shapes:
        n_in, n_out = s["n_in"], len(s["grid"])
        a, gp = _g(s["grid"])
        for P in (s["P"], s["P"] - 1, s["P"] // 4, 0, 1):
            for B in (s["B"], 1, 3):
                assert L.dpr_resolve_algo_sample_smooth_clouds(RASTER, n_in, n_out, gp, P, B) == _lib.ALGO_ATOMIC
                want = L.dpr_resolve_algo_smooth_clouds(RASTER, n_in, n_out, gp, P, B)
                assert want in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)
                got = L.dpr_resolve_algo_sample_smooth_clouds(PULLBACK, n_in, n_out, gp, P, B)
                assert got == want, (s["grid"], P, B)
                seen.add((n_out, got))
                if got == _lib.ALGO_TILED:  # only where the tiled path can run
                    assert L.dpr_workspace_bytes_sample_smooth_clouds_ex_f32(PULLBACK, 0, 0, n_in, n_out, gp, P,
                                                                             B) not in (0, SIZE_MAX)
        # the recorded choice of the splat's forward is this pullback's
        name = dpr_amd.resolve_algo_sample_smooth_clouds("pullback", s["grid"], s["P"], s["B"], n_in)
        assert name == s["auto"], (s["grid"], s["P"], s["B"])
        assert dpr_amd.resolve_algo_sample_smooth_clouds("sample", s["grid"], s["P"], s["B"], n_in) == "atomic"
    assert seen == {(n, a) for n in (2, 3) for a in (_lib.ALGO_ATOMIC, _lib.ALGO_TILED)}
    with pytest.raises(dpr_amd.DprError):
        dpr_amd.resolve_algo_sample_smooth_clouds("sample", (16, 16, 16), 10, 4, 2)


@pytest.mark.parametrize("suf,tdt", [("f32", torch.float32), ("f64", torch.float64)])
def test_workspace_bytes(suf, tdt):
    L = dpr_amd.lib()
    f = getattr(L, f"dpr_workspace_bytes_sample_smooth_clouds_ex_{suf}")
    splat = getattr(L, f"dpr_workspace_bytes_smooth_clouds_ex_{suf}")
    mpg = _lib.flag_max_pose_group
    for n_in, n_out in PAIRS:
        grid = (37, 19, 21) if n_out == 3 else (150, 37)
        a, gp = _g(grid)
        for flags in (0, mpg(1), mpg(2), mpg(16), _lib.FLAG_COHERENT_POINTS):
            for B in (1, 4, 64):
                for op in (RASTER, PULLBACK):
                    assert f(op, _lib.ALGO_ATOMIC, flags, n_in, n_out, gp, 1000, B) == 0
                assert f(RASTER, _lib.ALGO_AUTO, flags, n_in, n_out, gp, 1000, B) == 0
                assert f(PULLBACK, _lib.ALGO_AUTO, flags, n_in, n_out, gp, 1000, B) == 0  # (AUTO is ATOMIC here)
        # the TILED pullback: the workspace of the tiled forward of the smooth cloud splat, for the same flags
        sizes = set()
        for P in (1, 777, 20_000, 1_000_000):
            for B in (1, 5, 64):
                for n in (0, 1, 2, 16):
                    want = splat(RASTER, _lib.ALGO_TILED, mpg(n), n_in, n_out, gp, P, B)
                    assert want not in (0, SIZE_MAX)
                    assert f(PULLBACK, _lib.ALGO_TILED, mpg(n), n_in, n_out, gp, P, B) == want, (P, B, n)
                    sizes.add((P, B, want))
                    assert dpr_amd._pkg.workspace_bytes_sample_smooth_clouds("pullback", grid, P, B, n_in, tdt, "tiled",
                                                                        max_pose_group=n) == want
        assert len({w for _, _, w in sizes}) > 6  # (the group size does move the need)
        assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, 0, 4) == 0
        assert f(PULLBACK, _lib.ALGO_AUTO, 0, n_in, n_out, gp, 1_000_000, 4) == \
            splat(RASTER, _lib.ALGO_TILED, 0, n_in, n_out, gp, 1_000_000, 4)
        assert dpr_amd._pkg.workspace_bytes_sample_smooth_clouds("sample", grid, 1000, 4, n_in, tdt) == 0
        with pytest.raises(dpr_amd.DprError):
            dpr_amd._pkg.workspace_bytes_sample_smooth_clouds("sample", grid, 1000, 4, n_in, tdt, "tiled")
        with pytest.raises(ValueError):
            dpr_amd._pkg.workspace_bytes_sample_smooth_clouds("pullback", grid, 1000, 4, n_in, tdt, "tiled",
                                                         max_pose_group=17)
        assert f(PULLBACK, _lib.ALGO_TILED, 0, n_in, n_out, gp, (1 << 32) - 2, 1) != SIZE_MAX


@pytest.mark.parametrize("fid,kind,suf,op", FUNCTIONS, ids=[f[0] for f in FUNCTIONS])
def test_one_spoiled_argument(fid, kind, suf, op):
    """Every case of tests/smooth_refusal_cases.py for this family: bad pair, NULL grid, negative P / B, op 9 and the
    residual op, KEEP / REUSE, algorithms 3, 4, 9, a TILED forward, the four size bounds, P = 2^32 - 1 on TILED, each
    required pointer NULL, each pointer misaligned, every output NULL, the TILED workspace NULL / short / misaligned,
    and the empty call accepted."""
    L = dpr_amd.lib()
    rows = cases.spoils(L, FAMILY, kind, suf, op)
    labels = [label for label, _, _ in rows]
    assert len(labels) == len(set(labels))
    for want in ("pair (2,3)", "grid NULL", "P = -1", "B = -1", "P blocks too large", "B * P * n_in too large",
                 "G * B too large", "P * B too large"):
        assert want in labels
    if kind in ("query", "resolve"):
        assert "op = 9" in labels and "residual op" in labels
    if kind != "resolve":
        assert {"KEEP", "REUSE", "algo = 3", "algo = 4", "algo = 9"} <= set(labels)
        assert ("TILED" in labels) == (op == RASTER) and ("P = 2^32 - 1, TILED" in labels) == (op == PULLBACK)
    if kind == "bwd":
        assert {"every output NULL", "TILED, workspace NULL", "TILED, workspace short",
                "TILED, workspace misaligned", "no poses, no points"} <= set(labels)
        # (the grid, the five required pointers, every output, the workspace)
        assert sum(label.endswith(" NULL") for label in labels) == 1 + 5 + 2
        assert sum(label.endswith(" misaligned") for label in labels) == 9 + 1
    if kind == "fwd":
        assert sum(label.endswith(" NULL") for label in labels) == 5 + 1  # (and the grid)
        assert sum(label.endswith(" misaligned") for label in labels) == 5
    for label, over, says in rows:
        v, msg = cases.call(L, FAMILY, kind, suf, over)
        if says is None:
            assert v == _lib.OK, (label, v, msg)
            continue
        assert says in msg, (label, says, msg)
        if kind == "query":
            assert v == SIZE_MAX, (label, v, msg)
        else:
            assert v == _status(says), (label, v, msg)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_refusals_come_in_the_funnels_order(suf):
    """With two arguments spoiled the earlier check of csrc/dpr_host_smooth.h answers: pair, grid / P / B, op, size
    bounds, KEEP / REUSE, the algorithm, TILED on the forward, the workspace need of TILED; then the pointers:
    outputs, workspace, points, ds_dvalues and the poses, the image, alignment."""
    L = dpr_amd.lib()
    chains = {
        ("query", PULLBACK): [(dict(n_in=2, n_out=3), "(2,2), (3,3), (3,2)"), (dict(P=-1), "negative"),
                              (dict(op=9), "op 9"), (dict(B=1 << 51), "too large"), (dict(flags=cases.KEEP), "binning"),
                              (dict(algo=9), "algorithm 9")],
        ("fwd", RASTER): [(dict(n_in=2, n_out=3), "(2,2), (3,3), (3,2)"), (dict(grid=None), "grid is NULL"),
                          (dict(B=1 << 51), "too large"), (dict(flags=cases.REUSE), "binning"),
                          (dict(algo=cases.TILED), "ATOMIC only"), (dict(values=None), "values is NULL"),
                          (dict(image=None), "image is NULL"), (dict(points=None), "points is NULL"),
                          (dict(rot=cases.ODD), "aligned")],
        ("bwd", PULLBACK): [(dict(n_in=2, n_out=3), "(2,2), (3,3), (3,2)"), (dict(B=-1), "negative"),
                            (dict(P=1 << 40), "too large"), (dict(flags=cases.KEEP), "binning"),
                            (dict(algo=cases.ORDERED), "algorithm 4"),
                            (dict(ds_dimage=None, ds_dpoints=None, ds_drot=None, ds_dtrans=None), "every output"),
                            (dict(points=None), "points is NULL"), (dict(ds_dvalues=None), "ds_dvalues is NULL"),
                            (dict(trans=None), "rotation/translation"), (dict(image=None), "image is NULL"),
                            (dict(rot=cases.ODD), "aligned")],
    }
    for (kind, op), chain in chains.items():
        for i, (first, says) in enumerate(chain):
            for second, _ in chain[i + 1:]:
                if first.keys() & second.keys():
                    continue
                over = dict(dict(op=op), **first, **second)
                v, msg = cases.call(L, FAMILY, kind, suf, over)
                assert says in msg, (kind, first, second, msg)
                assert v == (SIZE_MAX if kind == "query" else _status(says)), (kind, first, second, v)
    # the workspace of TILED is looked at after the outputs and before the inputs
    v, msg = cases.call(L, FAMILY, "bwd", suf, dict(op=PULLBACK, algo=cases.TILED, points=None))
    assert v == _lib.ERR_WORKSPACE and "workspace" in msg
    # DPR_FLAG_MAX_POSE_GROUP is never refused: the forward and the ATOMIC pullback ignore it
    for kind, op in (("fwd", RASTER), ("bwd", PULLBACK)):
        v, msg = cases.call(L, FAMILY, kind, suf, dict(op=op, flags=cases.MPG2, B=0, P=0))
        assert v == _lib.OK, msg
        v, msg = cases.call(L, FAMILY, kind, suf, dict(op=op, flags=cases.MPG2, points=None))
        assert v == _lib.ERR_INVALID_ARG and "points is NULL" in msg
    # a pullback that does not ask for ds_dimage needs no workspace on TILED; without the image it needs no image
    v, msg = cases.call(L, FAMILY, "bwd", suf, dict(op=PULLBACK, algo=cases.TILED, ds_dimage=None, points=None))
    assert v == _lib.ERR_INVALID_ARG and "points is NULL" in msg
    v, msg = cases.call(L, FAMILY, "bwd", suf, dict(op=PULLBACK, image=None, ds_dpoints=None, ds_drot=None,
                                                    ds_dtrans=None, points=None))
    assert v == _lib.ERR_INVALID_ARG and "points is NULL" in msg


def test_python_wrappers_raise_without_a_device():
    B, P = 3, 10
    pts, img = torch.zeros(B, P, 3), torch.zeros(8, 8, 8, B)
    rot, trans = torch.eye(3).expand(B, 3, 3), torch.zeros(B, 3)
    dv = torch.zeros(B, P)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dpr_amd.sample_smooth_clouds(img, pts, rot, trans)
    pb = dpr_amd.sample_smooth_clouds_pullback_
    with pytest.raises(ValueError, match="unknown gradient"):
        pb(dv, img, pts, rot, trans, need=("weights",))
    with pytest.raises(ValueError, match="at least one"):
        pb(dv, img, pts, rot, trans, need=())
    with pytest.raises(ValueError, match="not in need"):
        pb(dv, img, pts, rot, trans, need=("image",), ds_dpoints=torch.zeros(B, P, 3))
    with pytest.raises(ValueError, match="only ds_dimage"):
        pb(dv, None, pts, rot, trans, grid_size=(8, 8, 8))
    with pytest.raises(ValueError, match="ds_dimage buffer or grid_size"):
        pb(dv, None, pts, rot, trans, need=("image",))
    with pytest.raises(ValueError, match="max_pose_group"):
        pb(dv, img, pts, rot, trans, max_pose_group=17)
    with pytest.raises(ValueError, match="max_pose_group"):
        dpr_amd.sample_smooth_clouds(img, pts, rot, trans, max_pose_group=-1)
    # shapes: those of per-pose clouds, the smooth pairs, and (B, P) values -- not the (P, B) of sample_smooth
    D = dpr_amd.DimensionMismatch
    with pytest.raises(D, match=r"\(B, P, N_in\)"):
        dpr_amd.sample_smooth_clouds(img, pts[0], rot, trans)
    with pytest.raises(D, match="batched poses"):
        dpr_amd.sample_smooth_clouds(img, pts, rot[0], trans[0])
    with pytest.raises(D, match="3 clouds, but rotation has 2 poses"):
        dpr_amd.sample_smooth_clouds_ad(img, pts, rot[:2], trans[:2])
    with pytest.raises(D, match="translation must be"):
        dpr_amd.sample_smooth_clouds(img, pts, rot, trans[:, :2])
    with pytest.raises(D, match="supports"):
        dpr_amd.sample_smooth_clouds(img, torch.zeros(B, P, 2), torch.zeros(B, 3, 2), trans)           # (2, 3)
    with pytest.raises(D, match="supports"):
        dpr_amd.sample_smooth_clouds_(dv, img, pts, torch.zeros(B, 1, 3), torch.zeros(B, 1))             # (3, 1)
    with pytest.raises(D, match=r"values must be \(B, P\)"):
        dpr_amd.sample_smooth_clouds_(torch.zeros(P, B), img, pts, rot, trans)
    with pytest.raises(D, match=r"ds_dvalues must be \(B, P\)"):
        pb(dv.t(), img, pts, rot, trans)
    # dtypes
    with pytest.raises(TypeError, match="promoted argument dtype"):
        dpr_amd.sample_smooth_clouds_(dv, img.double(), pts, rot, trans)
    with pytest.raises(TypeError, match="float32/float64"):
        dpr_amd.sample_smooth_clouds_(dv.half(), img.half(), pts.half(), rot.half(), trans.half())
    with pytest.raises(TypeError, match="torch.Tensor"):
        dpr_amd.sample_smooth_clouds(img, [[[0.0, 0.0, 0.0]]], rot[:1], trans[:1])
