// DPR_ALGO_TILED, host only: the slab cut of a grid, the workspace plan and the tiled_* queries of
// dpr_tiled.h.  No kernels here: an edit of the plan rebuilds in seconds.
#include <cstdlib>

#include "dpr_tiled_impl.h"

namespace dpr {

// tiles one launch sequence may hold: kMaxTiles, or less through DPR_MAX_TILES (read once; lets a
// test walk slabs on a small grid)
static int max_tiles() {
    static const int v = [] {
        const char* e = getenv("DPR_MAX_TILES");
        int x = e ? atoi(e) : kMaxTiles;
        return x < 16 ? 16 : (x > kMaxTiles ? kMaxTiles : x);
    }();
    return v;
}
template <int NO> bool make_slab_cut(const int64_t* grid, SlabCut* sc) {
    const int cap = max_tiles();  // tiles one launch sequence may hold (kMaxTiles unless DPR_MAX_TILES)
    int64_t per = 1;
    for (int d = 0; d + 1 < NO; ++d) per *= (grid[d] + TileDims<NO>::T[d] - 1) / TileDims<NO>::T[d];
    const int64_t layers = (grid[NO - 1] + TileDims<NO>::T[NO - 1] - 1) / TileDims<NO>::T[NO - 1];
    if (per > cap / 2 || layers > (1 << 20)) return false;  // (a real + a ghost layer must fit)
    sc->per_layer = (int)per;
    sc->layers = (int)layers;
    if (per * layers <= cap) {
        sc->lps = (int)layers;
        sc->nslab = 1;
    } else {
        sc->lps = (int)(cap / per) - 1;
        sc->nslab = (int)((layers + sc->lps - 1) / sc->lps);
    }
    return true;
}
// geometry of slab `s` (forward: with the ghost layer for s > 0)
template <int NO>
TileGeom<NO> slab_geom(const int64_t* grid, const SlabCut& sc, int s, bool forward) {
    TileGeom<NO> tg;
    for (int d = 0; d + 1 < NO; ++d)
        tg.nt[d] = (int)((grid[d] + TileDims<NO>::T[d] - 1) / TileDims<NO>::T[d]);
    const int first = s * sc.lps;
    const int real = (sc.layers - first < sc.lps) ? sc.layers - first : sc.lps;
    tg.ghost = (forward && s > 0) ? 1 : 0;
    tg.tz0 = first - tg.ghost;
    tg.nt[NO - 1] = real + tg.ghost;
    tg.NT = sc.per_layer * tg.nt[NO - 1];
    return tg;
}
// the largest tile count any slab of the cut has (what the workspace is planned for)
int slab_max_tiles(const SlabCut& sc) {
    return sc.nslab == 1 ? sc.per_layer * sc.layers : sc.per_layer * (sc.lps + 1);
}

// single-piece geometry (false: the grid needs slabs, or is beyond them)
template <int NO> static bool make_geom(const int64_t* grid, TileGeom<NO>* tg) {
    SlabCut sc;
    if (!make_slab_cut<NO>(grid, &sc) || sc.nslab != 1) return false;
    *tg = slab_geom<NO>(grid, sc, 0, true);
    return true;
}

template bool make_slab_cut<2>(const int64_t*, SlabCut*);
template bool make_slab_cut<3>(const int64_t*, SlabCut*);
template TileGeom<2> slab_geom<2>(const int64_t*, const SlabCut&, int, bool);
template TileGeom<3> slab_geom<3>(const int64_t*, const SlabCut&, int, bool);

// Pose groups: with few tiles per pose (2-D projections, small 3-D grids) the bins become
// (pose, tile) pairs of up to kMaxGroup poses, as long as they fit the write-combining
// scatter's 4096 LDS cursors: the points are read once per group instead of once per pose and
// the fixed per-launch costs (scans, halo pass, reductions, launch gaps) are shared.  Measured
// (tools/pose_group_probe.py): 10 M points -> 512^2, 485 -> 383 us per pose (fwd + bwd);
// 1 M points -> 128^3, 149 -> 65 us per pose.
// Memory: records and slot map are sized P * g (20 / 36 bytes per point-pose), so a group of g
// poses multiplies that part of the workspace by g -- bounded by P * g <= 2^27 (2.7 GB fp32,
// 4.8 GB fp64) and by the caller through DPR_FLAG_MAX_POSE_GROUP(n) (include/dpr.h).
constexpr int kMaxGroup = 16;
static int pose_group(int NT, int64_t P, int64_t B, int max_group) {
    const int limit = (max_group > 0 && max_group < kMaxGroup) ? max_group : kMaxGroup;
    int bg = 1;
    while (bg * 2 <= limit && bg * 2 <= B && NT * bg * 2 <= 4096 &&
           P * bg * 2 <= ((int64_t)1 << 27))  // records of a group: <= 2 GiB (fp32)
        bg *= 2;
    return bg;
}

PlanRequest plan_request(size_t elem, int op, unsigned flags, int n_in, int n_out, const SlabCut& sc, int64_t P,
                         int64_t B) {
    PlanRequest rq{};
    rq.elem = elem;
    rq.n_in = n_in;
    rq.n_out = n_out;
    rq.tiles = slab_max_tiles(sc);
    rq.P = P;
    rq.B = B;
    rq.max_group = max_pose_group(flags);
    rq.coherent = (flags & DPR_FLAG_COHERENT_POINTS) != 0;
    rq.share_batch = (flags & 3u) != 0;
    rq.slabbed = sc.nslab > 1;
    rq.fwd_only = op == DPR_OP_RASTER && !(flags & 3u);
    return rq;
}

Plan pose_plan(size_t elem, int n_in, int n_out, const SlabCut& sc, int64_t P) {
    return make_plan(PlanRequest{.elem = elem, .n_in = n_in, .n_out = n_out, .tiles = slab_max_tiles(sc), .P = P,
                                 .B = 1, .max_group = 1, .fwd_only = true});
}

Plan make_plan(const PlanRequest& rq) {
    const size_t elem = rq.elem;
    const int n_in = rq.n_in, n_out = rq.n_out, NT1 = rq.tiles;
    const int64_t P1 = rq.P, B = rq.B;
    const bool slabbed = rq.slabbed, fwd_only = rq.fwd_only;
    const bool coherent = rq.coherent && !slabbed;  // local binning keeps a batch's bins: one slab at a time cannot
    const bool share_batch = rq.share_batch && B > 1;
    const int max_group = share_batch ? 1 : rq.max_group;  // a kept binning is per pose
    Plan pl;
    pl.pose_stride = 0;
    pl.sort_inside = !coherent && NT1 > 4096 && B >= 4 && P1 >= 200000;
    // Local binning is per pose: a batch that forms pose groups (few tiles) keeps the
    // grouped pipeline, which reads the points once per group (10 M points -> 512^2, 4 poses:
    // 0.56 ms grouped, 0.63 ms pose by pose on local bins)
    pl.bg = pose_group(NT1, P1, B, max_group);
    pl.local = (coherent || pl.sort_inside) && !slabbed && NT1 <= kMaxLocalTiles &&
               pl.bg == 1;
    // poses binned by one k_bin_local launch (the points are read once for all of them): every
    // pose of a kept batch, else up to 8 -- each needs its own records, P * lb <= 2^29
    pl.lb = 1;
    if (pl.local && B > 1) {
        if (share_batch) {
            pl.lb = B < 16 ? (int)B : 16;  // (the B copies exist anyway)
        } else {
            pl.lb = B < 8 ? (int)B : 8;
            while (pl.lb > 1 && P1 * pl.lb > ((int64_t)1 << 29)) --pl.lb;
        }
    }
    pl.copies = share_batch ? B : pl.lb;
    const int NT = NT1 * pl.bg;          // bins
    const int64_t P = P1 * pl.bg;        // records
    // Slices of the cloud = blocks of k_count / the scatter = rows of the counts table.
    int64_t nblk, chunk;
    if (NT <= 4096) {
        // write-combining scatter (one workgroup per CU: its LDS): at most one slice per CU, so
        // that all of them run at once, and whole sub-chunks per slice (a partly filled round costs
        // as much as a full one; 3e6 points: 489 slices of 1.5 rounds -> 245 of 3: 0.131 -> 0.124 ms)
        const int64_t sub = (elem == 4) ? kWcPpt * kWcThreads : kWcPpt * kWcThreads / 2;
        chunk = ((P1 + 255) / 256 + sub - 1) / sub * sub;
        if (chunk < sub) chunk = sub;
    } else {
        nblk = (P1 + 8191) / 8192;
        if (nblk < 1) nblk = 1;
        if (nblk > kMaxBinBlocks) nblk = kMaxBinBlocks;
        chunk = (P1 + nblk - 1) / nblk;
        chunk = (chunk + kBinThreads - 1) / kBinThreads * kBinThreads;
        if (chunk < kBinThreads) chunk = kBinThreads;
    }
    nblk = (P1 + chunk - 1) / chunk;
    if (nblk < 1) nblk = 1;
    pl.nblk = (int)nblk;
    pl.chunk = chunk;
    // the layout: take(bytes) is the offset of the next region (regions start on 256-byte boundaries)
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes);
        return at;
    };
    pl.off_hdr = take(sizeof(BinHeader));  // what a KEEP_BINNING forward left, checked by a REUSE pullback
    pl.off_counts = take((size_t)nblk * NT * 4);
    pl.off_totals = take((size_t)NT * 4);
    pl.off_tile_start = take((size_t)(NT + 1) * 4);
    // split threshold: ~P/256 records (even a fully clustered cloud then yields >= 256 items,
    // one per CU, while the headline Gaussian cloud has no tile above it), at least 4096; a
    // split tile's parts hold more than cap/2 records each
    // (a forward call that keeps nothing for a pullback splits later: the parts of a split tile
    // cost the halo pass more than a 2x longer item costs the fixed-point tile kernel -- 1 M points
    // -> 128^3: forward 0.065 -> 0.059 ms; the pullback's gather prefers the finer split)
    int64_t cap = P / 256;
    const int64_t cap_min = fwd_only ? 2 * 4096 : 4096;
    if (cap < cap_min) cap = cap_min;
    if (n_out == 2) {
        // 2-D grids have few tiles (256 at 512^2) with cheap LDS tiles (8.7 KB): split
        // earlier so that a dense projection still gives the chip ~2048 items
        cap = P / 2048;
        if (cap < 2048) cap = 2048;
    }
    pl.cap = (uint32_t)cap;
    pl.max_slabs = (int)(2 * ((P + cap - 1) / cap) + 1);
    pl.max_items = NT + pl.max_slabs;
    pl.off_items = take((size_t)pl.max_items * sizeof(WorkItem));
    pl.off_nitems = take(4);  // [0] = items, [1] = record assignment of k_tile_splat, [2] / [3] = max / ~min |point_weight| bits
    pl.off_nzbins = take((size_t)kMaxBinBlocks * 4);  // bins touched per count block (k_count -> k_tilescan)
    pl.off_tparts = take((size_t)NT * 4);
    pl.off_tslab = take((size_t)NT * 4);
    pl.off_split = take((size_t)(pl.max_slabs / 2 + 2) * 4);  // [0] = n_split, [1..] = split tile ids (at most max_slabs / 2)
    pl.sub = elem == 4 ? 4096 : 2048;
    // The un-permute map in sorted order (dpr_tiled_impl.h, the layout): wherever one pose at a time goes
    // through the write-combining scatter and its gradient records are read once per point -- no pose
    // group, no local binning, no kept batch (whose poses are un-permuted together through slot_of[p]).
    pl.run_map = pl.bg == 1 && !pl.local && NT1 <= 4096 && pl.copies == 1;
    pl.nsub = (P1 + pl.sub - 1) / pl.sub;
    if (pl.nsub < 1) pl.nsub = 1;
    pl.max_desc = 0;
    int64_t nrec = P;  // records (+ spare slot for rejected points)
    if (pl.local) {
        pl.max_desc = pl.nsub * pl.sub;  // every sub-chunk owns `sub` descriptor slots ...
        nrec = pl.nsub * pl.sub;         // ... and a slab of `sub` records
        pl.off_ltot = take((size_t)(2 * NT1 + 2) * 4);  // (the cursors follow the totals directly: one clear covers both)
        pl.off_dcursor = take((size_t)NT1 * 4);
        pl.off_dstart = take((size_t)(NT1 + 1) * 4);
        pl.off_bdesc = take((size_t)pl.nsub * 4);
        pl.off_desc = take((size_t)pl.max_desc * sizeof(RunDesc));
        pl.off_sdesc = take((size_t)pl.max_desc * sizeof(RunDesc));
    }
    pl.off_rec = take((size_t)(nrec + 1) * 4 * elem);  // + spare slot for rejected points
    pl.off_idx = take((size_t)(P1 + 1) * 4);
    pl.off_slot = take((size_t)(P + 1) * 4);
    if (pl.copies > 1) {  // everything up to here exists once per pose (of a kept batch / a local batch)
        pl.pose_stride = o;
        o += (size_t)(pl.copies - 1) * pl.pose_stride;
    }
    pl.off_spts = pl.off_spw = pl.off_perm = pl.off_iperm = pl.off_sgrad = pl.off_sgradw = pl.off_sorttmp = o;
    if (pl.sort_inside) {
        pl.off_spts = take((size_t)P1 * n_in * elem);
        pl.off_spw = take((size_t)P1 * elem);
        pl.off_perm = o;  // (unused since the coarse cell sort: only the inverse is needed)
        pl.off_iperm = take((size_t)P1 * 4);  // inverse permutation: the un-sort of the gradients gathers through it
        pl.off_sgrad = take((size_t)P1 * n_in * elem);
        pl.off_sgradw = take((size_t)P1 * elem);
        pl.off_sorttmp = take(coarse_workspace_bytes(elem, P1));
    }
    pl.off_aux = o;
    // aux: forward = halo buffer | overflow slabs ; pullback = per-item partials
    const size_t nvh = (n_out == 3) ? tile_voxels_halo<3>() : tile_voxels_halo<2>();
    const size_t halo = align_up((size_t)NT * ((n_out == 3) ? halo_count<3>() : halo_count<2>()) * elem) +
                        align_up((size_t)pl.max_slabs * nvh * elem);
    const size_t partials = (size_t)pl.max_items * 16 * 8;
    o += align_up(halo > partials ? halo : partials);
    pl.total = o;
    return pl;
}

// Identity of a workspace layout: a REUSE_BINNING pullback must read the lists where -- and in
// the form in which -- the KEEP_BINNING forward wrote them.  The two calls compute their plans
// independently (DPR_FLAG_COHERENT_POINTS and DPR_FLAG_MAX_POSE_GROUP move regions), so the
// forward stores this id in the header and the pullback's kernels compare it on the device like
// the rest of the header.
uint32_t plan_layout_id(const Plan& pl) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a over the fields that place or shape the lists
    auto mix = [&](uint64_t v) {
        for (int i = 0; i < 8; ++i) {
            h ^= (v >> (8 * i)) & 0xffu;
            h *= 1099511628211ull;
        }
    };
    mix(pl.local ? 1 : 0);
    mix((uint64_t)pl.bg);
    mix((uint64_t)pl.sub);
    mix((uint64_t)pl.cap);
    mix(pl.off_items);
    mix(pl.off_rec);
    mix(pl.off_idx);
    mix(pl.off_slot);
    mix(pl.off_aux);
    mix(pl.local ? pl.off_sdesc : 0);
    mix(pl.pose_stride);
    mix(pl.off_iperm);
    mix((uint64_t)pl.lb);
    mix(pl.run_map ? kRunMapVersion : 0);  // (the form of the sorted map: a binning kept in another form is refused)
    const uint32_t id = (uint32_t)(h ^ (h >> 32));
    return id ? id : 1u;
}

static bool grid_cut(int n_out, const int64_t* grid, SlabCut* sc) {
    return n_out == 3 ? make_slab_cut<3>(grid, sc) : make_slab_cut<2>(grid, sc);
}

bool tiled_supported(int n_out, const int64_t* grid) {
    SlabCut sc;
    return grid_cut(n_out, grid, &sc);
}

// slabs the tiled path cuts the grid into (1: one piece; 0: not supported)
int tiled_slabs(int n_out, const int64_t* grid) {
    SlabCut sc;
    return grid_cut(n_out, grid, &sc) ? sc.nslab : 0;
}

bool tiled_preferred(int op, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t G) {
    (void)G;
    if (P >= (int64_t)1 << 32) return false;
    SlabCut sc;
    if (!grid_cut(n_out, grid, &sc)) return false;
    // A cloud that is SPARSE on the grid: the tiled path pays per tile (zeroing and flushing an LDS
    // tile, staging a ds_dout tile: ~25 ns each) whether points fall into it or not, the direct
    // kernels pay per point only.  Crossovers measured on 256^3 ... 768^3 and 2048^2 / 4096^2 with
    // 1e5 ... 1e7 points, 1 and 4 poses (tools/sparse_grid_probe.py, profiles/r04_sparse_grids.txt):
    // forward ~60 points per tile (3-D) / ~48 (2-D), pullback ~320 (3-D) / 150-430 (2-D) -- the
    // direct pullback only READS the cells its points touch.  Below that AUTO regretted up to 2.8x
    // (3e5 points -> 4096^2, pullback) with the thresholds that follow, which were fitted on grids
    // of up to 2048 tiles.
    const int64_t NT_all = (int64_t)sc.per_layer * sc.layers;
    const int64_t per_tile = op == DPR_OP_RASTER ? (n_out == 3 ? 60 : 48)
                                                 : (n_out == 3 ? 320 : (NT_all <= 4096 ? 150 : 430));
    if (P < per_tile * NT_all) return false;
    if (sc.nslab > 1) {
        // More than 32768 tiles (e.g. 1024^3): every slab re-reads the cloud, and the tile kernels
        // write the whole grid -- which the direct path's background fill does as well.  Forward:
        // the LDS tiles beat scattered global atomics from ~1e6 points on (1e7 points -> 1024^3:
        // measured in profiles/r04_experiments.md); the pullback's gathers are reads, the direct
        // kernel keeps them.
        return op == DPR_OP_RASTER && P >= 1000000;
    }
    const int NT = sc.per_layer * sc.layers;
    // Measured crossovers (profiles/r01_algo_sweep.txt: one pose; r01_algo_sweep_batched.txt:
    // 4-64 poses; 64^3 ... 256^3 and 128^2 / 512^2 grids).  One pose: the tiled pipeline's fixed
    // cost (6-7 launches) is repaid from ~2-3e5 points on, forward and backward alike.  Batched
    // poses on a grid that forms pose groups: the fixed cost is shared, the forward pays from
    // ~6e4 points; the direct pullback kernel, which keeps a point in registers across the poses
    // of a slice, stays ahead up to ~3e5 points (~6e5 when the grid is too large for groups).
    const bool grouped = B >= 4 && pose_group(NT, P, B, 0) >= 4;
    // (one pose on a small grid -- up to 256^2 or 128^3: from 1e5 points -- the direct kernel's atomics are
    // at most 1.25x ahead there on a cloud that fills the grid and 2x behind on a clustered one,
    // profiles/r03_auto_regret.txt)
    // (two or three poses: the same per pose -- 1e5 points x 2 poses -> 128^3: tiled 0.058 ms, direct 0.099)
    if (op == DPR_OP_RASTER && B < 4 && (NT <= 64 || (n_out == 3 && NT <= 256))) return P >= 100000;
    if (op == DPR_OP_RASTER) return P >= (grouped ? 60000 : 250000);
    if (B >= 4) return P >= (grouped ? 300000 : 600000);
    return P >= 250000;
}

// tiles per pose of the tiled path's geometry (of its largest slab; -1: not supported)
int tiled_tiles(int n_out, const int64_t* grid) {
    SlabCut sc;
    return grid_cut(n_out, grid, &sc) ? slab_max_tiles(sc) : -1;
}

// May a KEEP_BINNING / REUSE_BINNING pair with B > 1 poses share on the tiled path when
// DPR_ALGO_AUTO decides?  Every pose then keeps its own records (Plan::pose_stride): only where
// pose groups are not an option anyway (more than 2048 tiles per pose) and the kept records stay
// below ~21 GB at fp64, ~13 GB at fp32 (P * B <= 2^29: a 4-word record, a slot and an index per
// point and pose; independent of the element type, so that dpr_resolve_algo_ex needs none).  An
// explicit DPR_ALGO_TILED shares for any B.  Never on a grid that is processed in slabs (a slab's
// binning is overwritten by the next one).
bool tiled_batch_share_ok(int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (B < 2 || P < 1 || P * B > ((int64_t)1 << 29)) return false;
    SlabCut sc;
    if (!grid_cut(n_out, grid, &sc) || sc.nslab != 1) return false;
    return sc.per_layer * sc.layers * 2 > 4096;
}

int tiled_check(int n_out, const int64_t* grid, int64_t P, unsigned flags, const char* binning_flag, SlabCut* sc) {
    const bool quiet = !binning_flag;
    if (!grid_cut(n_out, grid, sc))
        return quiet ? DPR_ERR_UNSUPPORTED_ALGO
                     : fail(DPR_ERR_UNSUPPORTED_ALGO,
                            "DPR_ALGO_TILED: a tile layer of the grid has more than %d tiles", kMaxTiles / 2);
    if (P >= (int64_t)1 << 32)
        return quiet ? DPR_ERR_UNSUPPORTED_ALGO
                     : fail(DPR_ERR_UNSUPPORTED_ALGO, "DPR_ALGO_TILED: P must be < 2^32");
    if (sc->nslab > 1 && (flags & 3u))
        return quiet ? DPR_ERR_UNSUPPORTED_ALGO
                     : fail(DPR_ERR_UNSUPPORTED_ALGO,
                            "DPR_ALGO_TILED: a grid of more than %d tiles is processed in slabs, whose "
                            "binning cannot be kept (%s)", kMaxTiles, binning_flag);
    return DPR_OK;
}

size_t tiled_workspace_bytes(size_t elem, int op, unsigned flags, int n_in, int n_out,
                             const int64_t* grid, int64_t P, int64_t B) {
    (void)op;
    SlabCut sc;
    if (tiled_check(n_out, grid, P, flags, nullptr, &sc)) return (size_t)-1;  // refused by raster_tiled / pullback_tiled
    // (sized for the plan of a sharing pair / a pullback: a forward call that keeps nothing splits
    // heavy tiles later and needs no more than this -- so a workspace sized for `raster` serves every
    // call of the same problem, as before)
    return make_plan(plan_request(elem, DPR_OP_PULLBACK, flags, n_in, n_out, sc, P, B)).total;
}

// ------------------------------------------------------------------ channel forward and JVP: the one-pose plan
// (per-pose binning on a single-slab grid only: no pose groups, slabs or local binning)
bool pose_binning_cut(int n_out, const int64_t* grid, int64_t P, SlabCut* sc) {
    return tiled_check(n_out, grid, P, 0u, nullptr, sc) == DPR_OK && sc->nslab == 1;
}

bool tiled_channels_supported(int n_out, const int64_t* grid, int64_t P) {
    SlabCut sc;
    return pose_binning_cut(n_out, grid, P, &sc);
}

size_t channel_part_bytes(size_t elem, int64_t P, int C) {
    return align_up((size_t)C * (size_t)(P + 1) * elem) + align_up((size_t)C * 2 * 4);
}

size_t tiled_channels_workspace_bytes(size_t elem, int n_in, int n_out, const int64_t* grid, int64_t P,
                                      int64_t B, int C) {
    SlabCut sc;
    if (!pose_binning_cut(n_out, grid, P, &sc)) return (size_t)-1;
    // (at least the single-channel DPR_ALGO_TILED workspace of the batch: a workspace sized for the
    // single-channel call of the same shape plus the channel part always serves)
    size_t base = tiled_workspace_bytes(elem, DPR_OP_RASTER, 0u, n_in, n_out, grid, P, B);
    const size_t own = pose_plan(elem, n_in, n_out, sc, P).total;
    if (own > base) base = own;
    return base + channel_part_bytes(elem, P, C);
}

size_t jvp_part_bytes(size_t elem, int64_t P) {
    return align_up((size_t)(P + 1) * 4 * elem) + align_up(2 * 4);
}

size_t tiled_jvp_workspace_bytes(size_t elem, int n_in, int n_out, const int64_t* grid, int64_t P) {
    SlabCut sc;
    if (!pose_binning_cut(n_out, grid, P, &sc)) return (size_t)-1;
    return align_up(pose_plan(elem, n_in, n_out, sc, P).total) + jvp_part_bytes(elem, P);
}

}  // namespace dpr
