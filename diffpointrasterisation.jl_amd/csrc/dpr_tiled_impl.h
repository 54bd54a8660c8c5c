// DPR_ALGO_TILED, internal: the types, constants and plan functions that dpr_tiled.hip (kernels and
// drivers; it opens with the table of stages) and dpr_tiled_plan.hip (host only: slab cut, workspace
// plan, the tiled_* queries) share.  dpr_tiled.h is the interface to the rest of the library.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_device.h"
#include "dpr_jvp.h"
#include "dpr_run_map.h"
#include "dpr_tiled.h"

namespace dpr {

// ------------------------------------------------------------------ tile geometry
template <int NO> struct TileDims;
// 3-D tile shape and K4 block size (A/B measured on C3, profiles/r01_tile_shape_sweep.txt)
template <> struct TileDims<3> {
    static constexpr int T[3] = {64, 16, 8};
};
template <> struct TileDims<2> {
    static constexpr int T[3] = {32, 32, 1};
};
constexpr int kMaxTiles = 32768;     // LDS cursor table: 4 B per tile, <= 128 KiB
constexpr int kBinThreads = 1024;    // K1 / K3 block
constexpr int kWcThreads = 1024;     // block of the write-combining scatter
constexpr int kWcPpt = 4;            // points per thread of a write-combining sub-chunk (fp32)
constexpr int kSplatThreads = 512;   // forward tile kernel block
constexpr int kSplatRunsOcc = 4;     // waves per SIMD of k_tile_splat_runs: two blocks per CU
// fp64: the ds_dout tile is 80 KB, two workgroups per CU -- 512 threads each keep 16 waves on the CU
// as the fp32 kernel's four workgroups of 256 do (with 256: 2.3 waves per SIMD, half the wave time
// spent waiting; profiles/r04_c5_sq_counters.txt)
template <typename T> __host__ __device__ constexpr int gather_threads() {
    return sizeof(T) == 8 ? 512 : 256;
}
// waves per SIMD the pullback tile kernels are compiled for (fp64: 128 VGPRs, so that two
// workgroups of 512 fit a CU; fp32: four workgroups of 256 need no more than that either)
template <typename T> __host__ __device__ constexpr int gather_waves_per_simd() { return 4; }
constexpr int kUpb = 4;        // points per thread of the single-pose un-permute (a block = one scatter sub-chunk)
constexpr int kGatherRb = 8;   // rows of the ds_dout tile a wave requests before it stores the first
// (the pullback tile kernels run 4 workgroups = 16 waves per CU: their 40 KB ds_dout tile sets
// that, not the ~100 VGPRs)
constexpr int kMaxBinBlocks = 512;   // rows of the counts table (2 per CU)
constexpr int kSplitChunks = 8;      // k_halo_gather work items per split tile (3-D: kSplitRows tile rows each;
                                     // 2-D: 256 voxels a step of the flat loop)
constexpr int kSplitRows = 16;       // rows (l1, l2) of a 64 x 16 x 8 tile per work item
constexpr int kSplitGrid = 2048;     // ... and the blocks that walk them (idle blocks cost nothing
                                     // measurable: a grid limited to the live items changed no kernel time)

// Tile geometry of one launch sequence.  Grids of up to kMaxTiles tiles are one piece; larger
// ones are processed in SLABS along the last axis: `nt[NO-1]` tile layers starting at global layer
// `tz0`, the rest of the grid is invisible to the launch (points whose primary tile lies outside
// are treated like points outside the grid).  A forward slab other than the first starts with a
// GHOST layer (ghost = 1): the top layer of the slab below, binned and accumulated once more only
// for its upper halo -- the first real layer's low faces need it, and the slab below has long
// overwritten its halo buffer; ghost tiles flush no owned voxel and receive no halo.
template <int NO> struct TileGeom {
    int nt[NO];  // tiles per axis (of this slab)
    int NT;      // tiles per pose (of this slab)
    int tz0;     // first tile layer along the last axis
    int ghost;   // 1: local layer 0 is a ghost layer
};

template <int NO> __host__ __device__ constexpr int tile_voxels() {
    int v = 1;
    for (int d = 0; d < NO; ++d) v *= TileDims<NO>::T[d];
    return v;
}
template <int NO> __host__ __device__ constexpr int tile_voxels_halo() {
    int v = 1;
    for (int d = 0; d < NO; ++d) v *= TileDims<NO>::T[d] + 1;
    return v;
}
template <int NO> __host__ __device__ constexpr int halo_count() {
    return tile_voxels_halo<NO>() - tile_voxels<NO>();
}

// How a grid is cut into slabs: `per_layer` tiles in a layer of the last axis, `layers` layers,
// at most `lps` real layers per slab (a slab's tile count incl. a ghost layer stays <= kMaxTiles).
struct SlabCut {
    int per_layer, layers, lps, nslab;
};

// What a DPR_FLAG_KEEP_BINNING forward leaves at the start of the workspace, and what a
// DPR_FLAG_REUSE_BINNING pullback checks ON THE DEVICE before it trusts the work list, the
// records and the slot map: problem shape, element size, the identity of the point / weight
// buffers and the pose VALUES (bit patterns).  state: kBinValid after a KEEP forward, 0 after
// any other binning and after the pullback that consumed it (its gradient records overwrite
// the point records in place, so a second reuse must not pass).  A pullback that finds no
// matching header launches nothing that touches memory through the stale lists and returns
// NaN in every output (loud, not silent).
constexpr uint32_t kBinMagic = 0x44505242u, kBinValid = 1u;
struct alignas(16) BinHeader {
    uint32_t magic, state;
    uint32_t elem, n_in, n_out, has_pw;
    int64_t P;
    int32_t grid[3];
    uint32_t verdict;  // written by the consuming pullback's first kernel: 1 = header matched
    uint64_t points, pw;
    uint32_t layout, pad_[3];  // plan_layout_id() of the workspace layout the binning was written in
    unsigned char pose[96];  // rotation | translation bytes of pose 0 (<= 9 + 3 doubles)
};

// One unit of work of the tile kernels: a contiguous record range of one tile.  Tiles with
// more than `cap` records are split into several items (parts) so that a clustered cloud
// (few heavily loaded tiles) still fills the chip; the parts of a split tile leave their LDS
// tiles in overflow slabs that k_halo_gather sums.
struct alignas(16) WorkItem {
    uint32_t tile, begin, end;
    uint32_t part_nparts;  // part | nparts << 16
};

// ---- LOCAL BINNING (DPR_FLAG_COHERENT_POINTS) ------------------------------------------------
// For a spatially coherent cloud the per-pose permutation can stay LOCAL: a block orders one
// sub-chunk of S consecutive points by tile in LDS and writes it out as ONE contiguous run of
// records, plus a descriptor {tile, start, count} for every tile the sub-chunk touches (a
// handful -- 13 of 2048 for a 4096-point sub-chunk of the Hilbert-sorted C3 cloud).  No count
// pass over the points, no counts table, no column scan; the descriptors (3 % of the points'
// bytes) are sorted by tile instead of the records, and the tile kernels walk the record runs
// their descriptors name.  Correct for any order -- an incoherent cloud just yields about as
// many descriptors as points and runs slowly, which is why the caller has to ask for it.
struct alignas(8) RunDesc {
    uint32_t start;       // first record of the run
    uint32_t tile_count;  // tile | count << 15   (tile < 32768, count <= S <= 4096)
    __host__ __device__ uint32_t tile() const { return tile_count & 0x7fffu; }
    __host__ __device__ uint32_t count() const { return tile_count >> 15; }
};
constexpr int kMaxLocalTiles = 16384;  // tiles per pose local binning supports (its LDS histogram)
constexpr int kMaxRuns = 256;        // descriptors per round of a work item in k_tile_splat ...
constexpr int kMaxRunsGather = 64;   // ... and in k_tile_gather (their tables live in LDS: 4
                                     // gather blocks per CU leave room for 64 runs)

// Workspace layout (identical for raster and pullback so that a pullback can reuse the
// binning a raster call left behind, DPR_FLAG_KEEP_BINNING / DPR_FLAG_REUSE_BINNING):
//   counts table | totals | tile_start | work items, n_items, tile_parts, tile_slab | records | indices | slot_of | aux (halo / partials)
// What a pullback's un-permute finds in `indices` and `slot_of` (the sizes of the two regions never change):
//   slot_of[p]   = record slot of ORIGINAL point p, the spare slot for a rejected one; `indices` holds the
//                  point index of every record for the plain k_scatter with point weights, else nothing
//   run_map      (Plan::run_map: one pose at a time through the write-combining scatter) the map is kept in
//                  SORTED order and per record run instead (dpr_run_map.h has the format and both directions
//                  of it), per scatter sub-chunk of `sub` points starting at point g * sub:
//                  A run = the records of one tile inside one segment of 64 sorted positions.
//                    indices region, uint16 [g * sub + i] = owner word of sorted position i: the index inside
//                                                           the sub-chunk (< sub) of the point that owns it,
//                                                           bit 15 on the first position of a run; kRunNone
//                                                           from the first position no record owns (rejected
//                                                           points own none)
//                    slot_of region, uint32 [g * sub + 64 s + j] = record slot of the first record of run j of
//                                                           segment s; nothing from the segment's number of
//                                                           runs on
//                  2 + 4 * runs / sub bytes per point are written (3.2 at C3): the uint16 half fills at most
//                  half of `indices`, the run table a part of `slot_of` that depends on the cloud.
struct Plan {
    int bg;          // poses binned together (pose group, a power of two; 1 = per-pose pipeline)
    int nblk;
    int64_t chunk;
    uint32_t cap;    // records per work item above which a tile is split
    int max_items;   // NT + worst-case number of extra parts
    int max_slabs;   // overflow slabs (parts of split tiles)
    bool run_map;    // the pullback's map is kept in sorted order (see the layout above); part of plan_layout_id
    size_t off_hdr, off_counts, off_totals, off_tile_start, off_items, off_nitems, off_nzbins, off_tparts, off_tslab,
        off_split, off_rec, off_idx, off_slot, off_aux, total;
    // Cell sort of the cloud inside the call (dpr_coarse.h; batched poses on grids with more than
    // 4096 tiles): what local binning of all poses of a batch needs; up to 16384 tiles per pose --
    // beyond that the plain count / scatter pipeline runs on the cell-sorted copy
    bool sort_inside;
    size_t off_spts, off_spw, off_perm, off_iperm, off_sgrad, off_sgradw, off_sorttmp;
    // KEEP_BINNING / REUSE_BINNING with B > 1: every pose owns a copy of the per-pose part of the
    // layout (header ... slot map), pose_stride bytes apart, so that the pullback finds the binning
    // of EVERY pose of the forward call; 0 when the poses share one copy (nothing is kept)
    size_t pose_stride;
    // local binning (DPR_FLAG_COHERENT_POINTS, or the cloud cell-sorted inside the call; NT <= 16384)
    bool local;
    int lb;                // poses binned per k_bin_local launch (each into its own copy of the
                           // per-pose workspace: `copies` of them, pose_stride bytes apart)
    int64_t copies;
    int sub;               // points per sub-chunk
    int64_t nsub;          // sub-chunks = blocks of k_bin_local
    int64_t max_desc;      // descriptor slots: `sub` per sub-chunk
    size_t off_ltot, off_dstart, off_dcursor, off_bdesc, off_desc, off_sdesc;  // ltot: ndesc[NT] | npts[NT] | max|pw| | ~min|pw|
};

// ------------------------------------------------------------------ the plan (dpr_tiled_plan.hip)
// the slab cut of a grid (false: a tile layer alone is beyond one launch sequence), the geometry of slab
// `s` (forward: with the ghost layer for s > 0) and the largest tile count any slab of the cut has (what
// the workspace is planned for); NO = 2, 3
template <int NO> bool make_slab_cut(const int64_t* grid, SlabCut* sc);
template <int NO> TileGeom<NO> slab_geom(const int64_t* grid, const SlabCut& sc, int s, bool forward);
int slab_max_tiles(const SlabCut& sc);

// What a plan is made for.  raster_tiled, pullback_tiled and tiled_workspace_bytes decode the flags of a call
// in ONE place (plan_request): the layout must agree between a KEEP forward, the REUSE pullback and the query.
struct PlanRequest {
    size_t elem;
    int n_in, n_out;
    int tiles;         // tiles per pose (of the largest slab)
    int64_t P, B;
    int max_group;     // DPR_FLAG_MAX_POSE_GROUP (0: the library's limit)
    bool coherent;     // DPR_FLAG_COHERENT_POINTS
    bool share_batch;  // KEEP_BINNING / REUSE_BINNING: every pose keeps its binning
    bool slabbed;      // the grid is processed in slabs
    bool fwd_only;     // a forward call that keeps nothing for a pullback
};
// the request of a raster / pullback call (`op`: DPR_OP_RASTER or DPR_OP_PULLBACK) with `flags`
PlanRequest plan_request(size_t elem, int op, unsigned flags, int n_in, int n_out, const SlabCut& sc, int64_t P,
                         int64_t B);
Plan make_plan(const PlanRequest& rq);
// the single-channel plan of one pose (what a call with B = 1 and no flags runs): channel forward and JVP
Plan pose_plan(size_t elem, int n_in, int n_out, const SlabCut& sc, int64_t P);
uint32_t plan_layout_id(const Plan& pl);
// What raster_tiled, pullback_tiled and tiled_workspace_bytes refuse: DPR_OK and the slab cut, or
// DPR_ERR_UNSUPPORTED_ALGO.  `binning_flag` names the call's KEEP / REUSE flag in the message; NULL (the
// queries) records no message.
int tiled_check(int n_out, const int64_t* grid, int64_t P, unsigned flags, const char* binning_flag, SlabCut* sc);
// what the per-pose binning of the channel forward and the JVP runs on: a single-slab grid, P < 2^32
bool pose_binning_cut(int n_out, const int64_t* grid, int64_t P, SlabCut* sc);
// the caller's own part of the channel / JVP workspace (behind the plan's)
size_t channel_part_bytes(size_t elem, int64_t P, int C);
size_t jvp_part_bytes(size_t elem, int64_t P);

// workspace of the coarse cell sort (dpr_coarse.h, compiled in dpr_tiled.hip)
size_t coarse_workspace_bytes(size_t elem, int64_t P);

}  // namespace dpr
