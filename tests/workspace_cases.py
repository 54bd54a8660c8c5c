"""The table of workspace paths and the per-family plumbing behind tests/test_workspace_contract_table.py (CPU),
tests/test_workspace_contract_gpu.py and tests/test_families_streams_gpu.py.

A ROW is one path through a host driver that uses the caller's workspace: (family, op, algorithm, flags, grid, P, B),
the element types it has, its line in the read-before-write audit of DESIGN.md ("4.18 The workspace and stream
contract", column "id"), whether the audit found it clean enough for the all-ones pattern, and the outputs that
include/dpr.h's SUMMATION ORDER tables call bit-reproducible run to run -- each with the line of the table it rests
on.  A FAMILY knows how to make a problem on the host, put it on the device, allocate NaN outputs, call the entry
point on a given workspace and state the reference its own test module uses.

Shapes (include/dpr.h and the headers of csrc/ for the tile shapes): every grid has at least two tiles per axis and a
remainder tile under all of DPR_ALGO_TILED's 64 x 16 x 8 and 32 x 32, the owner tiles' 32 x 32 x 14, the chunk
lists' 32 x 16 x 8 and the smooth tiles' 16 x 8 x 8 and 64 x 16; P is no multiple of 256; the clouds are tests/data.py's
(0.4 * randn: about one point in ten has no cell under a pose, so rejected keys and spare slots are in play); point
weights lie in [0.5, 1.5), inside the 2^10 span of the fixed-point regime, so that the fp32 tiled and owner
forwards are exact and `==` can be asked of them.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import dpr_amd
from oracle import oracle
from tests import data as D
from tests import sample_smooth_reference as SSR
from tests import smooth_channels_reference as SCR
from tests import smooth_jvp_reference as JR
from tests import smooth_reference as SR
from tests.test_jvp_abi import jvp_reference, random_tangents
from tests.test_parity_gpu import grid_to_dev, tol

G3 = (70, 36, 18)    # 45 360 cells: three chunks of DPR_ORDERED_CELL_CHUNK
G2 = (70, 40)
G2_ORDERED = (150, 120)  # 18 000 cells: two cell chunks
P_SMALL = 3001           # a few thousand, 3001 = 11 * 256 + 185
P_CHUNKS = 9001          # 2-D DPR_ALGO_CHUNKED: two chunks of 4096 points and one of 809
P_ORDERED = 5001         # two chunks of DPR_ORDERED_POINT_CHUNK and one of 905
P_ONE_SLICE = 2001       # per-pose clouds on DPR_ALGO_CHUNKED: below 2048 points a cloud is one slice (clouds_plan)
C, K = 3, 2              # channels, tangents
NPDT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
PULLBACK_FIELDS = ("points", "rotation", "translation", "background", "out_weight", "point_weight")
KIND = dict(out="out", values="out", image="out", loss="out", points="points", point_weight="points",
            rotation="pose", translation="pose", background="pose", out_weight="pose")

# flag sets a row can carry (keyword arguments of the Python layer).  "local": DPR_FLAG_COHERENT_POINTS reaches the
# local binning of DPR_ALGO_TILED only where no pose group forms (Plan::local, csrc/dpr_tiled_plan.hip), so the
# row asks for one pose per group as well; the three poses are then binned by one launch into three pose copies.
FLAGS = {
    "": {},
    "local": dict(coherent_points=True, max_pose_group=1),
    "coherent": dict(coherent_points=True),
    "mpg1": dict(max_pose_group=1),
    "mpg2": dict(max_pose_group=2),
    "sharing": dict(sharing=True),
}

# ------------------------------------------------------------------ include/dpr.h, SUMMATION ORDER: the lines quoted
Q_TILED_OUT = "DPR_ALGO_TILED forward `out`: fp32: 64-bit fixed-point sums per tile, EXACT -- independent of the order " \
              "of the points and of execution"
Q_TILED_PTS = "DPR_ALGO_TILED ds_dpoints / ds_dpoint_weight: one gradient record per (point, pose), added per point " \
              "in a fixed order, group by group (note 2): bit-reproducible"
Q_OWNER_OUT = "DPR_ALGO_CHUNKED forward, 3-D owner tiles: fp32 EXACT (64-bit fixed point, split tiles summed as " \
              "integers) -- the same bits for any point order"
Q_OWNER_PTS = "DPR_ALGO_CHUNKED ds_dpoints / ds_dpoint_weight, 3-D: one thread per point, poses added in index order " \
              "...: bit-reproducible, the same bits for any point order"
Q_CO2D_POSE = "DPR_ALGO_CHUNKED per-pose sums, 2-D: the 4096 terms of a (chunk, pose) as a fixed tree in T ..., the " \
              "partials per (chunk, pose) in f64 in a fixed order, however the poses are sliced (ds_dbackground: " \
              "k_grid_sum, ... a fixed order up to 4096 cells)"
Q_ORDERED = "DPR_ALGO_ORDERED: NONE OF IT VARIES -- same bits run to run"
Q_CH_OUT = "channels, DPR_ALGO_TILED (forward only): fp32, fixed-point regime: every plane is BIT-IDENTICAL to the " \
           "single-channel DPR_ALGO_TILED call ... same binning, ... same per-channel scale and guard"
Q_SAMPLE_IMG = "PRECISION OF THE FIXED-POINT SUMS: POINT SAMPLING, ds_dimage on DPR_ALGO_TILED -- the pose: plane b " \
               "is the single-pose tiled forward with the column ds_dvalues[:, b] as its weights"
Q_CL_TILED_OUT = "per-pose clouds, DPR_ALGO_TILED: plane b = dpr_raster_ex_*(DPR_ALGO_TILED) of (cloud b, pose b), " \
                 "bit for bit"
Q_CL_TILED_PTS = "per-pose clouds, DPR_ALGO_TILED: ds_dpoints[b] = dpr_raster_pullback_ex_*(DPR_ALGO_TILED) of pose b"
Q_CL_CH_OUT = "per-pose clouds, DPR_ALGO_CHUNKED: fp32, one slice per (pose, tile): 64-bit fixed point per pose, EXACT -- " \
              "the same bits for any order of the cloud"
Q_CL_CH_PTS = "per-pose clouds, DPR_ALGO_CHUNKED: the owner tile of a (point, pose) stores it once: bit-reproducible"
Q_CL_CH_POSE = "per-pose clouds, DPR_ALGO_CHUNKED per-pose sums: ... partials summed in f64 in a fixed order: " \
               "bit-reproducible run to run (ds_dbackground: k_grid_sum's block atomics, rounding level on grids of " \
               "several blocks)"

BOTH, F32, F64 = ("f32", "f64"), ("f32",), ("f64",)


def _exact(names, dtypes, quote):
    return {n: (dtypes, quote) for n in names}


TILED_FWD = _exact(("out",), F32, Q_TILED_OUT)
TILED_BWD = _exact(("points", "point_weight"), BOTH, Q_TILED_PTS)
ORDERED_ALL = _exact(("out", "loss") + PULLBACK_FIELDS, BOTH, Q_ORDERED)
CO2D_BWD = _exact(("rotation", "translation", "out_weight", "background"), BOTH, Q_CO2D_POSE)  # (G2: 2800 cells)

Row = namedtuple("Row", "family op algo flags n_in grid P B dtypes audit poison exact")


def _rows():
    rows = []

    def add(family, op, algo, flags, n_in, grid, P, B, audit, exact=None, dtypes=BOTH, poison=True):
        rows.append(Row(family, op, algo, flags, n_in, tuple(grid), P, B, dtypes, audit, poison, exact or {}))

    core_ops = (("raster", TILED_FWD), ("pullback", TILED_BWD), ("residual_pullback", TILED_BWD))
    # DPR_ALGO_TILED: 3-D and 2-D (B = 3: pose groups of 2 + 1 poses), one pose per group, groups of two, local binning
    for n_in, grid in ((3, G3), (3, G2)):
        for op, exact in core_ops:
            add("core", op, "tiled", "", n_in, grid, P_SMALL, 3, "T1", exact)
    for op, exact in core_ops[:2]:  # (raster_residual_pullback_ has no max_pose_group keyword)
        add("core", op, "tiled", "mpg1", 3, G3, P_SMALL, 3, "T1", exact)
        add("core", op, "tiled", "mpg2", 3, G2, P_SMALL, 3, "T1", exact)
        add("core", op, "tiled", "local", 3, G3, P_SMALL, 3, "T2", exact)
    for op, exact in core_ops:
        add("core", op, "tiled", "coherent", 2, G2, P_SMALL, 3, "T1", exact)  # (pose groups form: the grouped path)
    # a KEEP forward, then the REUSE pullback and -- after a second KEEP forward -- the REUSE residual pullback, on
    # one buffer (every pose keeps its own binning)
    add("core", "pair", "tiled", "sharing", 3, G3, P_SMALL, 3, "T3", {**TILED_FWD, **TILED_BWD})
    # DPR_ALGO_CHUNKED on 3-D grids: owner tiles and the direct pullback (no residual variant), the chunk lists of a
    # sparse cloud over four poses (P * 10 <= G, B >= 4)
    add("core", "raster", "chunked", "", 3, G3, P_SMALL, 3, "O1", _exact(("out",), F32, Q_OWNER_OUT))
    add("core", "pullback", "chunked", "", 3, G3, P_SMALL, 3, "O2", _exact(("points", "point_weight"), BOTH, Q_OWNER_PTS))
    add("core", "raster", "chunked", "coherent", 3, G3, P_SMALL, 3, "O1", _exact(("out",), F32, Q_OWNER_OUT))
    add("core", "pullback", "chunked", "coherent", 3, G3, P_SMALL, 3, "O2",
        _exact(("points", "point_weight"), BOTH, Q_OWNER_PTS))
    add("core", "raster", "chunked", "", 3, G3, P_SMALL, 4, "O3")
    # DPR_ALGO_CHUNKED on 2-D grids: sorted inside the call, and on the caller's order (the partial sums only)
    # (the sort inside the call ranks the points of a cell with LDS atomics: the order inside a chunk, and with it
    # the bits of the fixed tree, are fixed only on the caller's own order)
    for flags, exact in (("", None), ("coherent", CO2D_BWD)):
        add("core", "raster", "chunked", flags, 3, G2, P_CHUNKS, 3, "C1")
        add("core", "pullback", "chunked", flags, 3, G2, P_CHUNKS, 3, "C1", exact)
        add("core", "residual_pullback", "chunked", flags, 3, G2, P_CHUNKS, 3, "C1", exact)
    # DPR_ALGO_ORDERED
    for n_in, grid in ((3, G3), (3, G2_ORDERED)):
        add("core", "raster", "ordered", "", n_in, grid, P_ORDERED, 3, "R1", ORDERED_ALL)
        add("core", "pullback", "ordered", "", n_in, grid, P_ORDERED, 3, "R2", ORDERED_ALL)
        add("core", "residual_pullback", "ordered", "", n_in, grid, P_ORDERED, 3, "R2", ORDERED_ALL)
    # the other families of the N-linear splat
    for n_in, grid in ((3, G3), (2, G2)):
        add("channels", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "T4", _exact(("out",), F32, Q_CH_OUT))
        add("sample", "pullback", "tiled", "", n_in, grid, P_SMALL, 3, "T1", _exact(("image",), F32, Q_SAMPLE_IMG))
        add("jvp", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "T5")
        add("clouds", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "T1", _exact(("out",), F32, Q_CL_TILED_OUT))
        add("clouds", "pullback", "tiled", "", n_in, grid, P_SMALL, 3, "T1",
            _exact(("points", "point_weight"), BOTH, Q_CL_TILED_PTS))
        # (fp64: no workspace.  3001 points are two slices of a cloud -- clouds_plan of csrc/dpr_api_clouds.hip cuts
        # a cloud into slices of at least 2048 points -- whose sums meet in float atomics: rounding level by the
        # table; 2001 points are one slice per (pose, tile), the EXACT case, held to ==)
        add("clouds", "raster", "chunked", "", n_in, grid, P_SMALL, 3, "L1", dtypes=F32)
        add("clouds", "raster", "chunked", "", n_in, grid, P_ONE_SLICE, 3, "L1", _exact(("out",), F32, Q_CL_CH_OUT),
            dtypes=F32)
        add("clouds", "pullback", "chunked", "", n_in, grid, P_SMALL, 3, "L2",
            {**_exact(("points", "point_weight"), BOTH, Q_CL_CH_PTS),
             **_exact(("rotation", "translation", "out_weight"), BOTH, Q_CL_CH_POSE)})
    # the smooth families: nothing on their tiled paths is bit-reproducible (float atomics in T across tiles)
    for n_in, grid in ((3, G3), (2, G2)):
        add("smooth", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "S1")
        add("sample_smooth", "pullback", "tiled", "", n_in, grid, P_SMALL, 3, "S1")
        add("smooth_jvp", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "S1")
        add("smooth_clouds", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "S2")
        add("smooth_channels", "raster", "tiled", "", n_in, grid, P_SMALL, 3, "S1")
    add("smooth_clouds", "raster", "tiled", "mpg2", 3, G3, P_SMALL, 3, "S2")  # groups of 2 + 1 poses: the last is smaller
    return rows


TABLE = _rows()


def row_id(row, dt):
    flags = f"+{row.flags}" if row.flags else ""
    return f"{row.family}-{row.op}-{row.algo}{flags}-{len(row.grid)}d-P{row.P}-B{row.B}-{dt}"


# ------------------------------------------------------------------ the public workspace queries
def _core_query(op, algo, flags, n_in, grid, P, B, tdt):
    return dpr_amd.workspace_bytes(op, grid, P, B, n_in, tdt, algo, **FLAGS[flags])


def _plain_query(fn):
    def q(op, algo, flags, n_in, grid, P, B, tdt):
        assert not flags
        return fn(op, grid, P, B, n_in, dtype=tdt, algo=algo)
    return q


def _extra_query(fn, extra):
    def q(op, algo, flags, n_in, grid, P, B, tdt):
        assert not flags
        return fn(op, grid, P, B, n_in, extra, dtype=tdt, algo=algo)
    return q


def _jvp_query(fn):
    def q(op, algo, flags, n_in, grid, P, B, tdt):
        assert not flags and op == "raster"
        return fn(grid, P, B, n_in, K, dtype=tdt, algo=algo)
    return q


def _smooth_clouds_query(op, algo, flags, n_in, grid, P, B, tdt):
    return dpr_amd.workspace_bytes_smooth_clouds(op, grid, P, B, n_in, dtype=tdt, algo=algo, **FLAGS[flags])


# public query function -> (family, the ops it takes, the flag sets that move its layout per algorithm, the query)
QUERIES = {
    "workspace_bytes": ("core", ("raster", "pullback", "residual_pullback"),
                        {"tiled": ("", "local", "coherent", "mpg1", "mpg2", "sharing"), "chunked": ("", "coherent")},
                        _core_query),
    "workspace_bytes_channels": ("channels", ("raster", "pullback"), {},
                                 _extra_query(dpr_amd.workspace_bytes_channels, C)),
    "workspace_bytes_sample": ("sample", ("raster", "pullback"), {}, _plain_query(dpr_amd.workspace_bytes_sample)),
    "workspace_bytes_jvp": ("jvp", ("raster",), {}, _jvp_query(dpr_amd.workspace_bytes_jvp)),
    "workspace_bytes_clouds": ("clouds", ("raster", "pullback"), {}, _plain_query(dpr_amd.workspace_bytes_clouds)),
    "workspace_bytes_smooth": ("smooth", ("raster", "pullback"), {}, _plain_query(dpr_amd.workspace_bytes_smooth)),
    "workspace_bytes_sample_smooth": ("sample_smooth", ("raster", "pullback"), {},
                                      _plain_query(dpr_amd.workspace_bytes_sample_smooth)),
    "workspace_bytes_smooth_jvp": ("smooth_jvp", ("raster",), {}, _jvp_query(dpr_amd.workspace_bytes_smooth_jvp)),
    "workspace_bytes_smooth_clouds": ("smooth_clouds", ("raster", "pullback"), {"tiled": ("", "mpg2")},
                                      _smooth_clouds_query),
    "workspace_bytes_smooth_channels": ("smooth_channels", ("raster", "pullback"), {},
                                        _extra_query(dpr_amd.workspace_bytes_smooth_channels, C)),
}
QUERY_OF = {family: q for family, _ops, _flags, q in QUERIES.values()}


def need_bytes(row, dt):
    """The workspace query of a row (the pair row: one buffer for the KEEP forward and both REUSE pullbacks)."""
    q = QUERY_OF[row.family]
    ops = ("raster", "pullback", "residual_pullback") if row.op == "pair" else (row.op,)
    return max(q(op, row.algo, row.flags, row.n_in, row.grid, row.P, row.B, TDT[dt]) for op in ops)


# ------------------------------------------------------------------ problems on the host
def _r(a, npdt):
    return np.ascontiguousarray(a, dtype=npdt)


@functools.lru_cache(maxsize=None)
def problem(family, n_in, grid, P, B, dt, seed):
    """Host arrays (in the element type) of one call of `family`; cached and read-only."""
    npdt = NPDT[dt]
    fam = family.replace("smooth_", "").replace("_smooth", "")
    d = D.make(n_points=P, n_in=n_in, n_out=len(grid), batch=B, grid_n=grid, seed=100 + seed, dtype=npdt)
    rng = np.random.default_rng(200 + seed)
    p = SimpleNamespace(family=family, dt=dt, grid=tuple(grid), P=P, B=B, n_in=n_in, n_out=len(grid),
                        points=d.points, rot=d.rotations, trans=d.translations, bg=d.backgrounds, ow=d.weights,
                        pw=_r(rng.uniform(0.5, 1.5, size=P), npdt), g=_r(d.ds_dout, npdt))
    if fam == "core":
        p.target = _r(rng.normal(size=p.grid + (B,)), npdt)
        p.out_img = oracle.raster(p.grid, p.points, p.rot, p.trans, p.bg, p.ow, p.pw, dtype=npdt)
    elif fam == "channels":
        p.pw = _r(rng.uniform(0.5, 1.5, size=(P, C)) * (1.0 + np.arange(C)), npdt)
        p.bg = _r(rng.uniform(-1, 1, size=(B, C)), npdt)
        p.g = _r(rng.normal(size=p.grid + (C, B)), npdt)
    elif fam == "sample":
        p.image = _r(rng.normal(size=p.grid + (B,)), npdt)
        p.dv = _r(rng.uniform(0.5, 1.5, size=(P, B)) * rng.choice([-1.0, 1.0], size=(P, B)), npdt)
    elif fam == "jvp":
        p.tan = {k: _r(v, npdt) for k, v in random_tangents(rng, K, P, B, n_in, p.n_out).items()}
    elif fam == "clouds":
        p.points = _r(np.stack([d.points, d.points[::-1] * 0.9, np.roll(d.points, 500, axis=0) * 1.1][:B] +
                               [d.points * 0.8] * max(0, B - 3)), npdt)
        p.pw = _r(rng.uniform(0.5, 1.5, size=(B, P)), npdt)
    for v in vars(p).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


# ------------------------------------------------------------------ families
def _dev(a, dev, image=False):
    """(a copy: the cached problems are read-only)  image: in the memory order of empty_grid"""
    a = np.array(a, order="C")
    return grid_to_dev(a, dev) if image else torch.as_tensor(a, device=dev)


def _nan(shape, tdt, dev):
    return torch.full(tuple(shape), float("nan"), dtype=tdt, device=dev)


def _nan_image(shape, tdt, dev):
    out = dpr_amd.empty_grid(tuple(shape[:-1]), shape[-1], tdt, dev)
    out.fill_(float("nan"))
    return out


def _nan_pullback(p, tdt, dev, pts_shape, pw_shape, bg_shape):
    return dict(points=_nan(pts_shape, tdt, dev), rotation=_nan((p.B, p.n_in, p.n_out), tdt, dev).transpose(1, 2),
                translation=_nan((p.B, p.n_out), tdt, dev), background=_nan(bg_shape, tdt, dev),
                out_weight=_nan((p.B,), tdt, dev), point_weight=_nan(pw_shape, tdt, dev))


def _pb_kwargs(out):
    return {f"ds_d{k}": out[k] for k in PULLBACK_FIELDS}


class Family:
    """images: the inputs kept in the memory order of empty_grid; algos: forward algorithm -> pullback algorithm."""
    images = ("g",)
    inputs = ("points", "rot", "trans", "bg", "ow", "pw", "g")
    ops = ("raster", "pullback")
    smooth = False

    def to_device(self, p, dev):
        return {k: _dev(getattr(p, k), dev, k in self.images) for k in self.inputs}

    def poses(self, inp):
        return inp["points"], inp["rot"], inp["trans"], inp["bg"], inp["ow"], inp["pw"]

    def outputs(self, op, p, dev):
        tdt = TDT[p.dt]
        if op == "raster":
            return dict(out=_nan_image(p.grid + (p.B,), tdt, dev))
        return _nan_pullback(p, tdt, dev, (p.P, p.n_in), (p.P,), (p.B,))


class Core(Family):
    images = ("g", "target", "out_img")
    inputs = Family.inputs + ("target", "out_img")
    ops = ("raster", "pullback", "residual_pullback")
    algos = {"atomic": "atomic", "tiled": "tiled", "chunked": "chunked", "ordered": "ordered"}

    def outputs(self, op, p, dev):
        out = super().outputs(op, p, dev)
        if op == "residual_pullback":
            out["loss"] = _nan((p.B,), TDT[p.dt], dev)
        return out

    def call(self, op, algo, flags, inp, out, ws):
        kw = {k: v for k, v in flags.items() if k != "sharing"}
        if op == "raster":
            dpr_amd.raster_(out["out"], *self.poses(inp), algo=algo, workspace=ws, **kw)
        elif op == "pullback":
            dpr_amd.raster_pullback_(inp["g"], *self.poses(inp), algo=algo, workspace=ws, **_pb_kwargs(out), **kw)
        else:
            loss = out["loss"]
            dpr_amd.raster_residual_pullback_(inp["out_img"], inp["target"], *self.poses(inp), scale=2.0, loss=loss,
                                              algo=algo, workspace=ws,
                                              **_pb_kwargs({k: out[k] for k in PULLBACK_FIELDS}), **kw)

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        if op == "raster":
            return dict(out=oracle.raster(p.grid, p.points, p.rot, p.trans, p.bg, p.ow, p.pw, dtype=npdt))
        if op == "pullback":
            return oracle.raster_pullback(p.g, p.points, p.rot, p.trans, p.ow, p.pw, dtype=npdt)._asdict()
        pb, loss = oracle.residual_pullback(p.out_img, p.target, p.points, p.rot, p.trans, p.ow, p.pw, scale=2.0,
                                            dtype=npdt)
        return dict(pb._asdict(), loss=loss.astype(npdt))


class Channels(Family):
    algos = {"atomic": "atomic", "tiled": "atomic"}  # (the pullback has DPR_ALGO_ATOMIC only)
    fwd, bwd = staticmethod(dpr_amd.raster_channels_), staticmethod(dpr_amd.raster_pullback_channels_)

    def outputs(self, op, p, dev):
        tdt = TDT[p.dt]
        if op == "raster":
            out = dpr_amd.empty_channel_grid(p.grid, C, p.B, tdt, dev)
            out.fill_(float("nan"))
            return dict(out=out)
        return _nan_pullback(p, tdt, dev, (p.P, p.n_in), (p.P, C), (p.B, C))

    def call(self, op, algo, flags, inp, out, ws):
        a = (inp["points"], inp["rot"], inp["trans"], inp["pw"], inp["bg"], inp["ow"])
        if op == "raster":
            self.fwd(out["out"], *a, algo=algo, workspace=ws)
        else:
            self.bwd(inp["g"], *a, algo=algo, workspace=ws, **_pb_kwargs(out))

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        if op == "raster":
            planes = [oracle.raster(p.grid, p.points, p.rot, p.trans, p.bg[:, c], p.ow, p.pw[:, c], dtype=npdt)
                      for c in range(C)]
            return dict(out=np.stack(planes, axis=-2))
        parts = [oracle.raster_pullback(p.g[..., c, :], p.points, p.rot, p.trans, p.ow, p.pw[:, c], dtype=npdt)
                 for c in range(C)]
        ref = {k: sum(getattr(r, k) for r in parts) for k in ("points", "rotation", "translation", "out_weight")}
        ref["background"] = np.stack([r.background for r in parts], axis=-1)
        ref["point_weight"] = np.stack([r.point_weight for r in parts], axis=-1)
        return ref


class SmoothChannels(Channels):
    smooth = True
    fwd = staticmethod(dpr_amd.raster_smooth_channels_)
    bwd = staticmethod(dpr_amd.raster_pullback_smooth_channels_)

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        if op == "raster":
            return dict(out=SCR.raster_smooth_channels(p.grid, p.points, p.rot, p.trans, p.pw, p.bg, p.ow).astype(npdt))
        ref = SCR.raster_pullback_smooth_channels(p.g, p.points, p.rot, p.trans, p.pw, p.ow)
        return {k: v.astype(npdt) for k, v in zip(PULLBACK_FIELDS, ref)}


class Sample(Family):
    images = ("image",)
    inputs = ("points", "rot", "trans", "image", "dv")
    algos = {"atomic": "atomic", "tiled": "tiled"}  # (forward algorithm of the "tiled" entry: atomic, see call)
    fwd, bwd = staticmethod(dpr_amd.sample_), staticmethod(dpr_amd.sample_pullback_)

    def to_device(self, p, dev):
        inp = super().to_device(p, dev)
        inp["dv"] = _dev(np.ascontiguousarray(p.dv.T), dev).t()  # (P, B), point index fastest
        return inp

    def outputs(self, op, p, dev):
        tdt = TDT[p.dt]
        if op == "raster":
            return dict(values=_nan((p.B, p.P), tdt, dev).t())
        return dict(image=_nan_image(p.grid + (p.B,), tdt, dev), points=_nan((p.P, p.n_in), tdt, dev),
                    rotation=_nan((p.B, p.n_in, p.n_out), tdt, dev).transpose(1, 2),
                    translation=_nan((p.B, p.n_out), tdt, dev))

    def call(self, op, algo, flags, inp, out, ws):
        a = (inp["image"], inp["points"], inp["rot"], inp["trans"])
        if op == "raster":  # (the forward has no tiled variant)
            self.fwd(out["values"], *a, algo="atomic", workspace=ws)
        else:
            self.bwd(inp["dv"], *a, algo=algo, workspace=ws, ds_dimage=out["image"], ds_dpoints=out["points"],
                     ds_drotation=out["rotation"], ds_dtranslation=out["translation"])

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        one = np.ones(1, npdt)
        pose = lambda b: (p.rot[b:b + 1], p.trans[b:b + 1])
        if op == "raster":
            return dict(values=np.stack([oracle.raster_pullback(p.image[..., b:b + 1], p.points, *pose(b), one,
                                                                dtype=npdt).point_weight for b in range(p.B)], axis=1))
        ref = dict(image=np.empty(p.grid + (p.B,), npdt), points=np.zeros((p.P, p.n_in), npdt),
                   rotation=np.empty((p.B, p.n_out, p.n_in), npdt), translation=np.empty((p.B, p.n_out), npdt))
        for b in range(p.B):
            ref["image"][..., b] = oracle.raster(p.grid, p.points, *pose(b), None, None, p.dv[:, b], dtype=npdt)[..., 0]
            r = oracle.raster_pullback(p.image[..., b:b + 1], p.points, *pose(b), one, p.dv[:, b], dtype=npdt)
            ref["rotation"][b], ref["translation"][b] = r.rotation[0], r.translation[0]
            ref["points"] += r.points
        return ref


class SampleSmooth(Sample):
    smooth = True
    fwd, bwd = staticmethod(dpr_amd.sample_smooth_), staticmethod(dpr_amd.sample_smooth_pullback_)

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        if op == "raster":
            return dict(values=SSR.sample_smooth(p.image, p.points, p.rot, p.trans).astype(npdt))
        ref = SSR.sample_smooth_pullback(p.dv, p.image, p.points, p.rot, p.trans)
        return {k: v.astype(npdt) for k, v in zip(("image", "points", "rotation", "translation"), ref)}


class Jvp(Family):
    ops = ("raster",)
    inputs = ("points", "rot", "trans", "bg", "ow", "pw")
    images = ()
    algos = {"atomic": None, "tiled": None}
    fwd = staticmethod(dpr_amd.raster_jvp_)
    TAN = ("points", "rotation", "translation", "background", "out_weight", "point_weight")

    def to_device(self, p, dev):
        inp = super().to_device(p, dev)
        inp.update({f"{k}_dot": _dev(p.tan[k], dev) for k in self.TAN})
        return inp

    def outputs(self, op, p, dev):
        out = dpr_amd.empty_channel_grid(p.grid, K, p.B, TDT[p.dt], dev)
        out.fill_(float("nan"))
        return dict(out=out)

    def call(self, op, algo, flags, inp, out, ws):
        self.fwd(out["out"], *self.poses(inp), tangents=K, algo=algo, workspace=ws,
                 **{f"{k}_dot": inp[f"{k}_dot"] for k in self.TAN})

    def reference(self, op, p):
        return dict(out=jvp_reference(p.grid, p.points, p.rot, p.trans, p.ow, p.pw, p.tan, K, cell_dtype=NPDT[p.dt]))


class SmoothJvp(Jvp):
    smooth = True
    fwd = staticmethod(dpr_amd.raster_smooth_jvp_)

    def reference(self, op, p):
        return dict(out=JR.raster_smooth_jvp(p.grid, p.points, p.rot, p.trans, p.ow, p.pw, K=K,
                                             **{f"{k}_dot": p.tan[k] for k in self.TAN}))


class Clouds(Family):
    algos = {"atomic": "atomic", "tiled": "tiled", "chunked": "chunked"}
    fwd, bwd = staticmethod(dpr_amd.raster_clouds_), staticmethod(dpr_amd.raster_pullback_clouds_)

    def outputs(self, op, p, dev):
        if op == "raster":
            return super().outputs(op, p, dev)
        return _nan_pullback(p, TDT[p.dt], dev, (p.B, p.P, p.n_in), (p.B, p.P), (p.B,))

    def call(self, op, algo, flags, inp, out, ws):
        if op == "raster":
            self.fwd(out["out"], *self.poses(inp), algo=algo, workspace=ws, **flags)
        else:
            self.bwd(inp["g"], *self.poses(inp), algo=algo, workspace=ws, **_pb_kwargs(out))

    def per_pose(self, op, p, b):
        npdt = NPDT[p.dt]
        a = (p.points[b], p.rot[b:b + 1], p.trans[b:b + 1])
        if op == "raster":
            return oracle.raster(p.grid, *a, p.bg[b:b + 1], p.ow[b:b + 1], p.pw[b], dtype=npdt)[..., 0]
        return tuple(oracle.raster_pullback(p.g[..., b:b + 1], *a, p.ow[b:b + 1], p.pw[b], dtype=npdt))

    def reference(self, op, p):
        parts = [self.per_pose(op, p, b) for b in range(p.B)]
        if op == "raster":
            return dict(out=np.stack(parts, axis=-1))
        ref = {k: np.concatenate([r[i] for r in parts]) for i, k in enumerate(PULLBACK_FIELDS)}
        ref["points"] = np.stack([r[0] for r in parts])
        ref["point_weight"] = np.stack([r[5] for r in parts])
        return ref


class SmoothClouds(Clouds):
    smooth = True
    algos = {"atomic": "atomic", "tiled": "atomic"}
    fwd = staticmethod(dpr_amd.raster_smooth_clouds_)
    bwd = staticmethod(dpr_amd.raster_pullback_smooth_clouds_)

    def per_pose(self, op, p, b):
        npdt = NPDT[p.dt]
        a = (p.points[b], p.rot[b:b + 1], p.trans[b:b + 1])
        if op == "raster":
            return SR.raster_smooth(p.grid, *a, p.bg[b:b + 1], p.ow[b:b + 1], p.pw[b])[..., 0].astype(npdt)
        return tuple(x.astype(npdt) for x in SR.raster_pullback_smooth(p.g[..., b:b + 1], *a, p.ow[b:b + 1], p.pw[b]))


class Smooth(Family):
    smooth = True
    algos = {"atomic": "atomic", "tiled": "atomic"}

    def call(self, op, algo, flags, inp, out, ws):
        if op == "raster":
            dpr_amd.raster_smooth_(out["out"], *self.poses(inp), algo=algo, workspace=ws)
        else:
            dpr_amd.raster_pullback_smooth_(inp["g"], *self.poses(inp), algo=algo, workspace=ws, **_pb_kwargs(out))

    def reference(self, op, p):
        npdt = NPDT[p.dt]
        if op == "raster":
            return dict(out=SR.raster_smooth(p.grid, p.points, p.rot, p.trans, p.bg, p.ow, p.pw).astype(npdt))
        ref = SR.raster_pullback_smooth(p.g, p.points, p.rot, p.trans, p.ow, p.pw)
        return {k: v.astype(npdt) for k, v in zip(PULLBACK_FIELDS, ref)}


FAMILIES = dict(core=Core(), channels=Channels(), sample=Sample(), jvp=Jvp(), clouds=Clouds(), smooth=Smooth(),
                sample_smooth=SampleSmooth(), smooth_jvp=SmoothJvp(), smooth_clouds=SmoothClouds(),
                smooth_channels=SmoothChannels())


@functools.lru_cache(maxsize=None)
def reference(family, op, n_in, grid, P, B, dt, seed):
    """name -> expected array (read-only, shared by the tests that need it)"""
    ref = FAMILIES[family].reference(op, problem(family, n_in, grid, P, B, dt, seed))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def tolerance(family, dt, name):
    """The tolerance the family's own test module holds `name` to (no new one): tests/test_parity_gpu.py's `tol`,
    which the channel, sampling, cloud and smooth modules share, and the two JVP modules' own."""
    npdt = NPDT[dt]
    if family == "jvp":
        from tests.test_jvp_gpu import tol as jvp_tol
        return jvp_tol(npdt)
    if family == "smooth_jvp":
        from tests.test_smooth_jvp_gpu import tol as smooth_jvp_tol
        return smooth_jvp_tol(npdt)
    return tol(npdt, KIND[name])
