/*
 * libdpr -- MI355X (gfx950) implementation of DiffPointRasterisation.jl's
 * `raster!` / `raster_pullback!` hot path behind a C ABI.
 *
 * This header is the drop-in boundary: the entry points are what a Julia
 * `DiffPointRasterisationAMDGPUExt` would `ccall` from array-type-specialised
 * methods of the reference's two canonical signatures (INTEGRATION.md shows the
 * binding):
 *
 *   dpr_raster_<T>           replaces  raster!  7-arg canonical method
 *                            /root/reference/src/raster.jl:5-34  (+ kernel :36-66)
 *   dpr_raster_pullback_<T>  replaces  raster_pullback!  13-arg batched method
 *                            /root/reference/src/raster_pullback.jl:85-148 and its
 *                            CUDA specialisation
 *                            /root/reference/ext/DiffPointRasterisationCUDAExt.jl:231-321
 *   (flat, un-slabbed output buffers as chosen by the allocator hooks at
 *    ext/DiffPointRasterisationCUDAExt.jl:323-333)
 *
 * Memory layouts are the reference's own (Julia column-major / AoS), so device
 * buffers can be passed without copies:
 *
 *   points        P x n_in AoS                      Vector{SVector{N_in,T}}
 *   rotation      B x (n_out x n_in, column-major)  Vector{SMatrix{N_out,N_in,T}}
 *   translation   B x n_out                         Vector{SVector{N_out,T}}
 *   background    B   or NULL => 0   (FillArrays.Zeros default, src/interface.jl:368-380)
 *   out_weight    B   or NULL => 1   (FillArrays.Ones  default, src/interface.jl:382-390)
 *   point_weight  P   or NULL => 1   (src/interface.jl:392-394)
 *   out, ds_dout  (n_1, .., n_N, B) column-major: axis 1 fastest, pose slowest
 *   ds_dpoints    n_in x P column-major (= AoS like points)
 *   ds_drotation  n_out x n_in x B column-major
 *   ds_dtranslation n_out x B ; ds_dbackground, ds_dout_weight: B ; ds_dpoint_weight: P
 *
 * All data pointers are DEVICE pointers owned by the caller (including the
 * workspace).  Calls only enqueue work on `stream` (a hipStream_t; NULL = the
 * default stream); they never synchronise the device and keep no device memory
 * or global state between calls.
 * THE STREAM CONTRACT.  Every entry point of every family only enqueues on `stream`, and can be
 * captured into a HIP graph: no synchronising call, no allocation, no launch or memset on another
 * stream, and what a captured call leaves in the graph is kernel nodes only (the library zeroes with
 * a kernel: the memset node of a captured hipMemsetAsync is not replayed reliably).
 * ONE EXCEPTION, refused and never silent: the paths that radix-sort -- DPR_ALGO_ORDERED's forward
 * (P keys per pose), the smooth families on DPR_ALGO_TILED (P keys per pose; per-pose clouds and rigid
 * bodies: P times the poses / images of a group), dpr_sort_points_* and the Hilbert sort inside 3-D DPR_ALGO_CHUNKED batches
 * and 2-D ones of more than 96 poses (P keys) -- use rocPRIM, whose sort of more than 2^20 keys
 * clears its histograms with hipMemsetAsync.  On a stream that is being captured such a call
 * returns DPR_ERR_HIP ("operation not permitted when stream is capturing"; kernels of the call in
 * front of the sort may already be nodes of the capture, which the caller discards).  Up to 2^20
 * keys these paths capture like the others, and outside a capture they run at any size.
 * Host threads may call concurrently, each on its own stream, outputs and workspace.
 * THE WORKSPACE CONTRACT (dpr_workspace_bytes_* below).  The initial contents of the workspace do
 * not matter: every piece of a layout is written by the call before the call reads it.  The
 * library writes only inside [workspace, workspace + workspace_bytes); with a workspace_bytes
 * equal to the query it uses no more.  What a call leaves in the workspace is unspecified, except
 * what a DPR_FLAG_KEEP_BINNING forward leaves for its DPR_FLAG_REUSE_BINNING pullback.
 * tests/test_workspace_contract_gpu.py and tests/test_families_streams_gpu.py hold every family to both
 * (SMOOTH SPLAT, RIGID BODIES, whose grouped layout is named piece by piece in its section:
 * tests/test_smooth_bodies_contract_gpu.py).
 * Supported (n_in, n_out): 1 <= n_in, n_out <= 4 in any
 * combination -- the reference is generic in both (src/raster.jl:5-13).
 * (2,2), (3,3), (3,2) -- the shapes the reference tests (src/raster.jl:112,
 * test/data.jl:13-19) -- have every algorithm; all other pairs (incl. n_out > n_in and 4-D) run on
 * DPR_ALGO_ATOMIC (what DPR_ALGO_AUTO resolves to for them) or, on request, DPR_ALGO_ORDERED; the other
 * algorithms and the KEEP / REUSE flags return DPR_ERR_UNSUPPORTED_ALGO.
 *
 * Error behaviour: the reference throws DimensionMismatch / ArgumentError before
 * any launch (src/raster.jl:14-23, ext/...CUDAExt.jl:246-262).  Here every entry
 * point returns a status (0 = ok) and records a message retrievable with
 * dpr_last_error() (thread-local); nothing is launched on error.
 */
#ifndef DPR_H
#define DPR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPR_VERSION 110 /* 0.1.10: + DPR_ALGO_ORDERED (bit-reproducible raster and pullback) */

/* status codes */
#define DPR_OK 0
#define DPR_ERR_UNSUPPORTED_DIMS (-1) /* not 1 <= n_in, n_out <= 4 */
#define DPR_ERR_INVALID_ARG (-2)      /* NULL required pointer, negative size, bad grid */
#define DPR_ERR_WORKSPACE (-3)        /* workspace NULL/too small for the chosen algorithm */
#define DPR_ERR_HIP (-4)              /* a HIP runtime call failed */
#define DPR_ERR_UNSUPPORTED_ALGO (-5) /* algorithm not available for this shape */

/* operations, for dpr_workspace_bytes_* and dpr_resolve_* */
#define DPR_OP_RASTER 0
#define DPR_OP_PULLBACK 1
/* the pullback entered through dpr_raster_residual_pullback_*: with DPR_ALGO_AUTO it never resolves to the
 * 3-D DPR_ALGO_CHUNKED pullback (which has no residual variant), so its workspace can differ from
 * DPR_OP_PULLBACK's for the same shape -- query with this op before a residual call */
#define DPR_OP_RESIDUAL_PULLBACK 2

/* algorithms (the *_ex entry points; the plain ones use DPR_ALGO_AUTO) */
#define DPR_ALGO_AUTO 0
#define DPR_ALGO_ATOMIC 1 /* thread per point, direct global float atomics / gathers */
#define DPR_ALGO_TILED 2  /* per-pose binning of points into voxel tiles, LDS-resident
                             tile accumulation (fp32 data: exact 64-bit fixed-point sums, scale
                             from |out_weight| * max|point_weight|; NaN / Inf weights and fp64
                             data: f64 sums), plain-store flush (no global atomics).  Grids of
                             more than 32768 tiles (e.g. 1024^3) are walked in slabs of tile
                             layers along the last axis -- no KEEP / REUSE there; a single tile
                             layer of more than 16384 tiles is DPR_ERR_UNSUPPORTED_ALGO.
                             AUTO picks it from ~2.5e5 points on where the cloud is dense enough
                             on the grid (the path costs ~25 ns per tile, with or without points
                             in it): >= 60 points per tile for the forward (48 on 2-D grids),
                             >= 320 for the pullback (150-430 on 2-D grids). */
#define DPR_ALGO_CHUNKED 3 /* chunks of consecutive points of a spatially coherent cloud.
                              2-D grids (projections; what AUTO picks for several poses of a
                              cloud, by a cost model -- dpr_resolve_algo_ex): a
                              block owns a chunk of 4096 points and an LDS tile under its
                              small projected footprint, and loops over the poses -- forward:
                              LDS accumulation + row-shaped global atomic flush, pullback:
                              LDS-staged ds_dout, gradients in registers across poses, no
                              atomics.  Unless DPR_FLAG_COHERENT_POINTS says the cloud is coherent
                              it is sorted into the workspace first (a counting sort into 4096
                              Hilbert-numbered cells for up to 96 poses, a radix sort on 15-bit
                              Hilbert keys beyond: compact 4096-point chunks are what the kernels
                              need, not sorted neighbours).
                              3-D grids: three kernel families behind one name.  FORWARD:
                              voxel tiles of 32 x 32 x 14 cells that own their cells outright
                              (no halo exchange, no global atomics, exact 64-bit fixed-point sums
                              for fp32 data) and find their points through a hierarchy of
                              grid-frame boxes over groups of 16 / 1024 / 65536 consecutive
                              points, built per call by one pass over the cloud -- no per-point
                              record is written; a cloud that is SPARSE on the grid (P * 10 <= G)
                              over >= 4 poses runs small 32 x 16 x 8 tiles fed by per-tile lists
                              of 64-point chunks instead.  PULLBACK: a thread per point in cloud
                              order gathers its eight ds_dout cells straight from memory (no
                              workspace beyond the partial sums: 0.9 MB per pose, 64 poses at
                              most); batches run the pose loop inside the kernel, 64 poses per
                              launch.
                              What AUTO picks with DPR_FLAG_COHERENT_POINTS: the owner-tile
                              forward for >= 2 poses of a DENSE cloud (0.4 <= P / G <= 2) on a
                              grid of >= 1024 such tiles (256^3: 1216); the chunk-list forward
                              for >= 4 poses of a sparse cloud (P >= 30000, P * 10 <= G from 16
                              poses on, P * 25 <= G for 4..15 poses); the pullback for one pose
                              from 1e4 points on, for 2..31 poses from P >= G / 28, for any
                              number of poses from 3e6 points (1e6 on grids of <= 1024 tiles of
                              DPR_ALGO_TILED).  KEEP / REUSE flags are dropped where the pullback
                              is this one (it reads nothing a forward could leave).
                              Without the flag, from 8 poses and 2e5 points on, the 3-D calls
                              Hilbert-sort the cloud into the workspace themselves (the workspace
                              query says how much more that takes) and AUTO picks them for large
                              batches: the pullback from 16 poses of 3e6 points on (8 of 1e7, 64 of
                              1e6), the forward from 32 poses of a dense cloud of 3e6 points and
                              from 16 poses of a sparse one (P * 10 <= G) of 2e5 points.
                              Correct for any point order.
                           */
#define DPR_ALGO_ORDERED 4 /* every sum in a FIXED order: all seven outputs (out, the six gradients) and the
                              residual's loss are bit-reproducible -- run to run, device to device, whatever
                              B and wherever the pose stands in the batch (SUMMATION ORDER below).  Opt-in:
                              DPR_ALGO_AUTO never resolves to it.  For dpr_raster_ex_*, dpr_raster_pullback_ex_*
                              and dpr_raster_residual_pullback_ex_*, both element types, every (n_in, n_out)
                              with 1 <= n_in, n_out <= 4, any B.  No floating-point atomics.
                              FORWARD, pose by pose: a 32-bit key per point (its reference cell on the grid
                              extended by one cell on the low side of every axis; all ones for a rejected
                              point), a stable radix sort of (key, point index) on the key bits that grid
                              needs, a start table over the extended grid (a lower-bound search per entry),
                              then one thread per output cell merges the <= 2^N index-sorted lists of its
                              source cells by point index and adds the one neighbour of each point that
                              lands on the cell, starting from the background: the forward is BIT-IDENTICAL
                              to the serial reference order (pose, point, neighbour).
                              PULLBACK: one thread per point, the pose loop over ALL poses inside the thread
                              (never sliced, never atomic); per-pose sums through fixed chunks (below).
                              COST: a cell's sum is serial by contract, so the forward's time grows with the
                              most populated cell (a thread adds its cell's contributions one after another);
                              a cloud concentrated on a few cells runs at the speed of those cells.
                              LIMITS (DPR_ERR_UNSUPPORTED_ALGO, (size_t)-1 from the workspace query): the
                              extended grid, prod (n_d + 1), must have at most 2^32 - 1 cells, and
                              P <= 2^32 - 2.  Workspace: forward 16 P bytes + the sort's temporary storage
                              + 4 (prod (n_d + 1) + 1) bytes, independent of B (0 for P = 0); pullback 8 bytes
                              per (point chunk, pose, scalar) and 16 per (cell chunk, pose).
                              FLAGS: KEEP / REUSE are refused (nothing to keep), COHERENT_POINTS and
                              MAX_POSE_GROUP are accepted and ignored, NO_POINT_WEIGHT_GRAD is honoured.
                              The other op families (channels, sampling, JVP, per-pose clouds) do not have
                              it: DPR_ERR_UNSUPPORTED_ALGO. */
/* The multi-channel entry points (MULTI-CHANNEL below) run DPR_ALGO_ATOMIC or, for the forward,
   DPR_ALGO_TILED: AUTO takes DPR_ALGO_TILED where the single-channel rule above prefers it for the shape
   and the grid is one slab, DPR_ALGO_ATOMIC otherwise (always for the pullback).
   The sampling entry points (SAMPLING below) run DPR_ALGO_ATOMIC for the forward; their pullback takes
   DPR_ALGO_TILED where the single-pose forward of the shape would, DPR_ALGO_ATOMIC otherwise.
   The per-pose cloud entry points (PER-POSE CLOUDS below) run DPR_ALGO_ATOMIC, DPR_ALGO_TILED (the single-pose
   tiled calls, pose by pose) or DPR_ALGO_CHUNKED (pose-owned LDS tiles). */

/* Chunk sizes of DPR_ALGO_ORDERED's per-pose sums (compile-time constants; the reduction trees depend on
 * nothing else): consecutive points per partial of ds_drotation / ds_dtranslation / ds_dout_weight, consecutive
 * cells of a plane per partial of ds_dbackground / loss. */
#define DPR_ORDERED_POINT_CHUNK 2048
#define DPR_ORDERED_CELL_CHUNK 16384

/* SUMMATION ORDER.  The reference promises none for its float atomics (src/raster.jl:64) and sums
 * serially per pose on the CPU (src/raster_pullback.jl:39-72).  Here, per algorithm and output:
 *
 *   algorithm            forward `out`                           ds_dpoints / ds_dpoint_weight         per-pose sums (ds_drotation, ds_dtranslation,
 *                                                                                                       ds_dout_weight, ds_dbackground)
 *   DPR_ALGO_ATOMIC      global float atomics: depends on the    one thread per point.  Pose loop      wave -> block -> one float atomic per block:
 *                        execution order (varies run to run,     inside the thread (B == 1, or         varies run to run at rounding level
 *                        rounding level)                         P >= 524 033): bit-reproducible,
 *                                                                the bits of the serial reference.
 *                                                                Otherwise the poses are sliced:
 *                                                                rounding level (note 1)
 *   DPR_ALGO_TILED       fp32: 64-bit fixed-point sums per       one gradient record per (point,       per-thread sums in T over the tile's records
 *                        tile, EXACT -- independent of the       pose), added per point in a fixed     (their order in the tile's list varies), then
 *                        order of the points and of execution;   order, group by group (note 2):       f64 across threads and tiles in a fixed order:
 *                        tiles split into parts (> max(4096,     bit-reproducible, the same bits for   rounding level of T within a tile
 *                        P/256) records) add their parts in      any order of the points
 *                        fp32 in a fixed order, the records
 *                        of a part vary: rounding level.
 *                        fp64: f64 LDS atomics, order-dependent
 *                        at 1e-16 relative
 *   DPR_ALGO_CHUNKED     2-D: exact fixed-point sums per chunk   2-D: registers across the poses of     2-D: the 4096 terms of a (chunk, pose) as a
 *                        (fp32; note 3), then float atomics      a chunk.  All poses in one block       fixed tree in T (fp32 data; fp64: f64 across
 *                        into the image across chunks: run to    (B == 1, or P >= 4 190 209 and         threads), the partials per (chunk, pose) in f64
 *                        run, rounding level.  3-D owner tiles:  B <= 64): bit-reproducible, the same   in a fixed order, however the poses are sliced
 *                        fp32 EXACT (64-bit fixed point, split   bits wherever the point stands in the  (ds_dbackground: k_grid_sum, one float atomic per
 *                        tiles summed as integers) -- the same   cloud.  Otherwise the poses are        4096 cells -- a fixed order up to 4096 cells).
 *                        bits for any point order; fp64: f64     sliced: rounding level (note 1).       3-D: per-thread sums in T over a slice of the cloud
 *                        LDS atomics, rounding level.  3-D       3-D: one thread per point, poses       (its size follows the CU count of the device), then
 *                        chunk lists (sparse clouds): f64 LDS    added in index order (registers        f64.  One pose: a fixed order.  Batches (pose loop
 *                        atomics + diverted global atomics       across a launch of <= 64 poses,        inside): fp64 ds_drotation / ds_dtranslation /
 *                                                                memory between launches): bit-         ds_dout_weight in a fixed order; fp32 data, and
 *                                                                reproducible, the same bits for any    ds_dbackground of either type, add their waves'
 *                                                                point order                            sums with f64 LDS atomics in arrival order:
 *                                                                                                       rounding level of f64
 *   DPR_ALGO_ORDERED     starts as background[b]; the            one thread per point, accumulators     the cloud cut into chunks of DPR_ORDERED_POINT_CHUNK
 *                        contributions voxel_weight(dlo, s,      start at 0, poses added in index       consecutive points; a chunk's terms reduced in T by
 *                        ow * pw) that land on a cell are added   order; never sliced over poses,        a fixed tree (sub-steps of 256 points: wave_sum,
 *                        one at a time, in T, in ascending        never atomic: the bits of the serial   waves in index order; sub-steps in order); the chunk
 *                        point index (a point reaches a cell      reference (oracle_raster_pullback)     partials added in f64 in ascending chunk order and
 *                        through at most one neighbour): the                                             rounded to T once.  ds_dbackground and the residual's
 *                        order and the BITS of the serial                                                loss: the same over chunks of DPR_ORDERED_CELL_CHUNK
 *                        reference (oracle_raster), fp32 and                                             consecutive cells of plane b.  Nothing depends on B,
 *                        fp64; independent of launch geometry,                                           the pose's index, a slice count or the CU count:
 *                        device, B and the pose's index                                                  NONE OF IT VARIES -- same bits run to run, and for
 *                                                                                                       a pose alone or anywhere inside a batch
 *
 *   channels (dpr_raster_channels_ex_* / dpr_raster_pullback_channels_ex_*, see MULTI-CHANNEL below):
 *   DPR_ALGO_TILED       fp32, fixed-point regime: every plane
 *   (forward only)       is BIT-IDENTICAL to the single-channel
 *                        DPR_ALGO_TILED call with point_weight[c, :]
 *                        and background[c, :] for B = 1 -- same
 *                        binning, same split of heavy tiles (> cap
 *                        records), same per-channel scale and guard.
 *                        Exceptions, at rounding level: a tile split
 *                        into parts (its parts' records vary run to
 *                        run in the single-channel call as well), and
 *                        B > 1 where the single-channel call bins
 *                        pose groups or cell-sorts the cloud (a
 *                        different cap / record order of split tiles).
 *                        A channel whose guard trips (or fp64 data):
 *                        f64 LDS atomics, as the single-channel call
 *   DPR_ALGO_ATOMIC      global float atomics, each contribution     one thread per point, channels folded  as DPR_ALGO_ATOMIC; the channels are
 *                        the single-channel value: rounding level    per gather.  Pose loop inside the      folded per gather before the sums:
 *                                                                    thread (B == 1, or P >= 524 033):      rounding level
 *                                                                    bit-reproducible; otherwise the poses
 *                                                                    are sliced: rounding level (note 1)
 *
 *   per-pose clouds (dpr_raster_clouds_ex_* / dpr_raster_pullback_clouds_ex_*, see PER-POSE CLOUDS below):
 *   DPR_ALGO_ATOMIC      global float atomics: rounding level        one thread per (point, pose), one      wave -> block -> one float atomic per block:
 *                                                                    plain store: bit-reproducible; B = 1   rounding level
 *                                                                    = dpr_raster_pullback_ex_* ATOMIC
 *   DPR_ALGO_TILED       plane b = dpr_raster_ex_*(DPR_ALGO_TILED)   ds_dpoints[b] = dpr_raster_pullback_   those of the single-pose tiled pullback of
 *                        of (cloud b, pose b), bit for bit           ex_*(DPR_ALGO_TILED) of pose b         pose b
 *   DPR_ALGO_CHUNKED     fp32, one slice per (pose, tile): 64-bit    the owner tile of a (point, pose)      per-thread sums in T over a fixed set of
 *                        fixed point per pose, EXACT -- the same     stores it once: bit-reproducible       points, f64 across waves, one partial per
 *                        bits for any order of the cloud; several                                           workgroup, partials summed in f64 in a fixed
 *                        slices: float atomics across slices,                                               order: bit-reproducible run to run
 *                        rounding level; fp64 / guard tripped:                                              (ds_dbackground: k_grid_sum's block atomics,
 *                        f64 LDS atomics, rounding level                                                    rounding level on grids of several blocks)
 *
 *   smooth splat (dpr_raster_smooth_ex_* / dpr_raster_pullback_smooth_ex_*, see SMOOTH SPLAT below):
 *   DPR_ALGO_ATOMIC      global float atomics in T, in arrival      one thread per point.  Pose loop       wave -> block -> one float atomic per block:
 *                        order: rounding level                       inside the thread (B == 1, or          rounding level
 *                                                                    P >= 524 033): one thread adds all
 *                                                                    poses in index order, one plain
 *                                                                    store: bit-reproducible.  Otherwise
 *                                                                    the poses are sliced: rounding level
 *                                                                    (note 1)
 *   DPR_ALGO_TILED       f64 LDS atomics within a tile (arrival
 *   (forward only)       order, 1e-16 relative), rounded to T once
 *                        per (tile, cell); a cell receives <= 3^N
 *                        such partials as float atomics in T onto
 *                        the background: rounding level, not
 *                        bit-reproducible
 *
 *   smooth splat, per-pose clouds (dpr_raster_smooth_clouds_ex_* / dpr_raster_pullback_smooth_clouds_ex_*, see SMOOTH
 *   SPLAT, PER-POSE CLOUDS below):
 *   DPR_ALGO_ATOMIC      global float atomics in T, in arrival      one thread per (point, pose), one      wave -> block -> one float atomic per block:
 *                        order: rounding level                       plain store per value, no slices, no   rounding level
 *                                                                    accumulation: bit-reproducible
 *   DPR_ALGO_TILED       as the smooth splat's tiled forward per
 *   (forward only)       (pose, tile), whatever the pose groups:
 *                        f64 LDS atomics in arrival order, rounded
 *                        to T once per (tile, cell), <= 3^N such
 *                        partials per cell as float atomics in T:
 *                        rounding level, not bit-reproducible
 *
 *   smooth splat, C weights per point (dpr_raster_smooth_channels_ex_* / dpr_raster_pullback_smooth_channels_ex_*, see
 *   SMOOTH SPLAT, MULTI-CHANNEL below), per channel / plane:
 *   DPR_ALGO_ATOMIC      as the smooth splat's, into plane (c, b):   as the smooth splat's, pose slices      as the smooth splat's; a thread adds its
 *                        rounding level                              alike (note 1).  One slice: one thread  C channels in index order before the wave
 *                                                                    adds all poses and, for ds_dpoints,     sum: rounding level
 *                                                                    all channels in index order, one plain
 *                                                                    store per value: bit-reproducible
 *   DPR_ALGO_TILED       as the smooth splat's tiled forward per
 *   (forward only)       (tile, channel): f64 LDS atomics in arrival
 *                        order, rounded to T once per (tile, cell,
 *                        channel), <= 3^N such partials per cell as
 *                        float atomics in T: rounding level, not
 *                        bit-reproducible
 *
 *   smooth splat, rigid bodies (dpr_raster_smooth_bodies_ex_* / dpr_raster_pullback_smooth_bodies_ex_*, see SMOOTH SPLAT,
 *   RIGID BODIES below):
 *   DPR_ALGO_ATOMIC      global float atomics in T, in arrival      as the smooth splat's, image slices     ds_drotation / ds_dtranslation per (image, body):
 *                        order: rounding level                       alike (note 1).  One slice (B == 1, or  a block of one body wave -> block -> one float
 *                                                                    P >= 524 033): one thread adds all      atomic per value; otherwise a masked wave sum
 *                                                                    images in index order, one plain        per body of the wave, one float atomic per value
 *                                                                    store: bit-reproducible; K = 1, B = 1:  and body.  ds_dout_weight wave -> block -> one
 *                                                                    the bits of the smooth splat's ATOMIC   float atomic per block; ds_dbackground as
 *                                                                    pullback                                everywhere: rounding level
 *   DPR_ALGO_TILED       as the smooth splat's tiled forward per
 *   (forward only)       (image, tile), whatever the groups and
 *                        the order of the bodies: f64 LDS atomics
 *                        in arrival order, rounded to T once per
 *                        (tile, cell), <= 3^N such partials per
 *                        cell as float atomics in T: rounding
 *                        level, not bit-reproducible
 *
 *   smooth splat, forward mode (dpr_raster_smooth_jvp_ex_*, see SMOOTH SPLAT, FORWARD MODE below), out_dot:
 *   DPR_ALGO_ATOMIC      global float atomics in T onto the background tangent, unordered: rounding level (lanes of
 *                        a wave with the same centre cell are first added in T in a fixed order, one atomic per group)
 *   DPR_ALGO_TILED       f64 LDS sums per (tile, tangent) in arrival order, rounded to T once per (tile, cell); a
 *                        cell receives <= 3^N such partials as float atomics in T onto the background tangent:
 *                        rounding level, not bit-reproducible
 *
 *   smooth sampling of C-channel images (dpr_sample_smooth_channels_ex_* / dpr_sample_smooth_channels_pullback_ex_*, see
 *   SMOOTH SAMPLING, MULTI-CHANNEL below):
 *   values               no sum across threads, no atomics: plane (c, b) in the order of SMOOTH SAMPLING -- the BITS of
 *                        dpr_sample_smooth_ex_* on that plane, fp32 and fp64
 *   ds_dpoints           a thread adds its C channels in index order, then the poses of its slice in index order; one
 *                        slice: one plain store, bit-reproducible; several: float atomics, rounding level (note 1)
 *   per-pose sums        the C channels in index order inside the thread, then wave -> block -> one float atomic per
 *                        block: rounding level
 *   ds_dimage            DPR_ALGO_ATOMIC: global float atomics in T, unordered: rounding level.  DPR_ALGO_TILED: the
 *                        smooth channel splat's tiled forward per (pose, tile, channel): rounding level
 *
 * Note 1, pose slices.  A per-point kernel that would leave the device idle cuts the B poses into slices on
 * the second grid axis; every slice adds its share of ds_dpoints / ds_dpoint_weight with float atomics onto
 * zeroed buffers.  DPR_ALGO_ATOMIC and its channel form: fewer than 2048 blocks of 256 points (P <= 523 776)
 * and B > 1 give up to min(B, ceil(2048 / blocks)) slices; from 2048 blocks on (P >= 524 033) one slice, whatever B.
 * 2-D DPR_ALGO_CHUNKED: a slice holds pps = min(64, ceil(B / s)) poses, with s = min(B, ceil(1024 / chunks)) below
 * 1024 chunks of 4096 points (P <= 4 190 208) and s = 1 from there on, and there are ceil(B / pps) slices.  A block
 * never takes more than 64 poses, so one slice needs B == 1, or P >= 4 190 209 and B <= 64; at P >= 4 190 209,
 * 65 <= B <= 128 gives two slices and B >= 129 three or more -- B >= 129 is sliced at any P.
 * From three slices on the arrival order decides the bits: rounding level, varies run to run.  Two slices give
 * the same bits run to run (two shares onto zero commute), but in general not those of the serial order.  A
 * point that every pose rejects keeps the +0 of the memset.  Callers who need the bits: DPR_ALGO_ORDERED.
 * Note 2, pose groups.  DPR_ALGO_TILED adds a point's records in index order within a group of poses binned
 * together (16 / 8 / 4 / 2 / 1 poses by the grid's tile count and DPR_FLAG_MAX_POSE_GROUP; up to 8 poses of a
 * DPR_FLAG_COHERENT_POINTS batch on local bins) and then adds the groups' sums in index order: for groups of
 * 4 + 2 + 1 poses (g0 + g1 + g2 + g3) + (g4 + g5) + g6.  A batch whose binning was kept (KEEP / REUSE) and
 * DPR_FLAG_MAX_POSE_GROUP(1) add pose by pose, ((g0 + g1) + g2) + ...: the same bits as each other, and as the
 * grouped sum only while no group after the first holds more than one pose.
 * Note 3, fixed-point forwards.  "EXACT" and "exact fixed-point sums" (DPR_ALGO_TILED, both DPR_ALGO_CHUNKED forwards,
 * fp32) hold in the fixed-point regime: the non-zero |point_weight| of the scope within a span of 2^10, none NaN / Inf
 * (PRECISION OF THE FIXED-POINT SUMS below; NULL weights always).  A scope with wider weights sums with IEEE f64
 * atomics: rounding level, like fp64 data.
 *
 * "Rounding level" = the differences any two summation orders of the same terms show in the
 * accumulation type; no output depends on the order beyond that.  The contributions themselves
 * (cell choice, weights) are computed with the reference's operation order in T and do not depend
 * on any order.
 *
 * PRECISION OF THE FIXED-POINT SUMS (fp32 data; the reference's float atomics, src/raster.jl:62-64, keep
 * the relative precision of every cell whatever its magnitude).  A contribution is rounded to a multiple of
 * 2^-sexp, with sexp chosen per work item so that n * maxw * 2^sexp <= 2^62 (n = records of the item,
 * maxw = |out_weight| * max |point_weight| of the SCOPE: the call on DPR_ALGO_TILED, the candidate chunks of
 * a tile on the 3-D DPR_ALGO_CHUNKED forward, the 4096-point chunk on the 2-D one): a contribution keeps at
 * least 38 bits below maxw (items hold < 2^24 records; typically 49).  Where the NON-ZERO |point_weight| of
 * a scope span more than 2^10 -- or a weight is NaN / Inf -- the scope accumulates with IEEE f64 atomics
 * instead (since 0.1.5; before, cells reached only by points lighter than ~2^-38 of the call's heaviest came
 * out as 0).  So every contribution keeps >= 28 bits (typically 39) below the SMALLEST weight next to it,
 * and a cell's absolute error is <= k * 2^-39 * (smallest weight in scope) for its k contributions: below
 * fp32 rounding (2^-24 relative) for every cell except far corners of their only contributors (value below
 * ~2^-12 of the local weight), which keep at least 16 good bits.  Default weights (NULL) never trip the guard.
 * tests/test_parity_gpu.py::test_fp32_cells_reached_only_by_small_weights_keep_their_relative_precision.
 * The scopes of the other op families (each takes maxw and the guard from its own scope, never from the one
 * before it in the call): MULTI-CHANNEL on DPR_ALGO_TILED -- the channel of a pose, |point_weight[c, :]| of the
 * points that pose bins; FORWARD-MODE DERIVATIVE on DPR_ALGO_TILED -- the (pose, tangent), with the bound
 * m_p = |a| + sum_n |b_n| of a record in the place of |point_weight| (out_weight is part of a and b_n);
 * POINT SAMPLING, ds_dimage on DPR_ALGO_TILED -- the pose: plane b is the single-pose tiled forward with the
 * column ds_dvalues[:, b] as its weights; PER-POSE CLOUDS on DPR_ALGO_CHUNKED -- the guard per pose, over the
 * whole cloud point_weight[b, :] (points outside the grid included), the scale per (pose, tile, slice).
 * tests/test_families_precision_gpu.py holds every one of them to a per-cell bound relative to the weights that
 * reach the cell.
 *
 * ENVIRONMENT.  DPR_MAX_TILES is the only variable the library reads (16..32768, default 32768): the number
 * of tiles DPR_ALGO_TILED handles per launch sequence before it cuts the grid into slabs along the last axis
 * -- a test hook that lets a small grid walk the slab code; it moves slab boundaries, never results. */

/* flags (the *_ex entry points).  DPR_ALGO_TILED: any B -- with B > 1 every pose keeps its own
 * binning (the per-pose part of the workspace is laid out B times; pose groups are off);
 * DPR_ALGO_CHUNKED on 2-D grids: any B (what is kept there is the sorted copy of the cloud and its
 * permutation); 3-D DPR_ALGO_CHUNKED: accepted and ignored (its pullback reads nothing a forward
 * could leave); DPR_ALGO_ATOMIC has nothing to keep (error):
 * KEEP_BINNING  (raster)   leave the per-tile binning of the points (incl. original
 *                          indices) in the workspace for the pullback of the same call pair
 * REUSE_BINNING (pullback) the workspace still holds the binning written by the preceding
 *                          raster call with the SAME points, pose, grid and point_weight
 *                          pointer-ness; skips the count/scan/scatter stages.
 * This is the cache an rrule keeps between `raster` and its pullback closure
 * (ext/DiffPointRasterisationChainRulesCoreExt.jl:6-27); the reference itself recomputes
 * (src/raster_pullback.jl:20-22). */
#define DPR_FLAG_KEEP_BINNING 1u
#define DPR_FLAG_REUSE_BINNING 2u
/* A REUSE_BINNING pullback validates ON THE DEVICE that the workspace holds the binning of a
 * KEEP_BINNING forward with the same P, grid, element type, points / point_weight buffers and
 * pose values, and that no pullback has consumed it yet (the gradient records overwrite the
 * point records), and that it was written in the workspace LAYOUT of this call (same
 * DPR_FLAG_COHERENT_POINTS / DPR_FLAG_MAX_POSE_GROUP on both calls of the pair).  If not, nothing
 * is read through the stale lists and the outputs come back as NaN; the status is still 0
 * because the host cannot see the mismatch without synchronising.  Which outputs: DPR_ALGO_TILED
 * -- all six and `loss`; DPR_ALGO_CHUNKED on 2-D grids (what is reused there is the sorted copy of
 * the cloud) -- ds_dpoints, ds_dpoint_weight, ds_drotation, ds_dtranslation and ds_dout_weight,
 * while ds_dbackground and `loss` do not depend on the points and stay valid.
 *
 * DPR_FLAG_MAX_POSE_GROUP(n), n in 1..16 (0 = library default 16): DPR_ALGO_TILED bins up to n
 * poses of a batch together when the grid has few tiles (n * tiles <= 4096).  Larger groups are
 * faster (the points are read once per group) but the record / slot-map part of the workspace
 * grows n-fold: (20 | 36) bytes * P * n for fp32 | fp64 -- e.g. 10 M points, 512^2 grid:
 * 0.28 GB at n = 1, 1.66 GB at n = 8.  Pass the same flags to dpr_workspace_bytes_ex_*. */
#define DPR_FLAG_MAX_POSE_GROUP(n) (((unsigned)(n) & 0xffu) << 8)
/* DPR_FLAG_COHERENT_POINTS: the caller states that neighbouring points in memory are
 * neighbours in space (e.g. the output of dpr_sort_points_*).  DPR_ALGO_CHUNKED on 2-D grids
 * then skips its own Hilbert sort (and the workspace shrinks to the per-pose partial sums);
 * DPR_ALGO_TILED bins such a cloud locally (sub-chunks of 4096 / 2048 consecutive points ordered
 * by tile in LDS, run descriptors instead of a count pass; grids of up to 16384 tiles) and, for a
 * batch, all poses of up to 8 in one launch.  Without the flag batched calls on grids of more than
 * 4096 tiles order the cloud themselves first (a counting sort into 4096 cells of the model frame,
 * once per call).  A wrong claim costs speed, never correctness. */
#define DPR_FLAG_COHERENT_POINTS 4u
/* DPR_FLAG_NO_POINT_WEIGHT_GRAD (pullback entry points): the caller does not need
 * ds_dpoint_weight -- the reference's rrule drops that tangent whenever `point_weight` was
 * defaulted (ext/DiffPointRasterisationChainRulesCoreExt.jl:23,70).  The pointer may be NULL and
 * nothing is written through it (a P-element store per call less; every algorithm honours it).
 * The five other outputs are unchanged. */
#define DPR_FLAG_NO_POINT_WEIGHT_GRAD 8u

int dpr_version(void);

/* Thread-local message of the last failing call on this host thread ("" if none). */
const char *dpr_last_error(void);

/* Algorithm DPR_ALGO_AUTO resolves to for this problem (DPR_ALGO_ATOMIC, DPR_ALGO_TILED or, on
 * 2-D grids, DPR_ALGO_CHUNKED), or a negative status.  The choice depends on the flags:
 *  - DPR_FLAG_COHERENT_POINTS makes the paths that exploit it cheaper;
 *  - with DPR_FLAG_KEEP_BINNING or DPR_FLAG_REUSE_BINNING the choice is made for the raster +
 *    pullback PAIR (both calls must run the same algorithm), from arguments both calls share.
 *    When the pair's algorithm has nothing to share (DPR_ALGO_ATOMIC; DPR_ALGO_TILED with
 *    B > 1 on a grid small enough for pose groups, or with more than 2^29 (point, pose) pairs
 *    to keep), AUTO ignores the two flags -- each call then works on its own -- where an
 *    explicitly named algorithm returns an error (DPR_ALGO_ATOMIC) or shares at any size
 *    (DPR_ALGO_TILED: every pose of the batch keeps its own binning, B-fold workspace).  So a caller may always pass AUTO + KEEP to
 *    raster and AUTO + REUSE to the pullback of the same arguments.
 * dpr_resolve_algo is dpr_resolve_algo_ex with flags = 0. */
int dpr_resolve_algo(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
int dpr_resolve_algo_ex(int op, unsigned flags, int n_in, int n_out, const int64_t *grid,
                        int64_t P, int64_t B);
/* The flags DPR_ALGO_AUTO will act on for this problem (>= 0), or a negative status: `flags`
 * with DPR_FLAG_KEEP_BINNING / DPR_FLAG_REUSE_BINNING cleared where the pair's algorithm has
 * nothing to share.  A host that wants to know whether the pullback will really skip its binning
 * (e.g. to report it) asks here. */
int dpr_resolve_flags_ex(int op, unsigned flags, int n_in, int n_out, const int64_t *grid,
                         int64_t P, int64_t B);

/* Optional per-stage device timing (used by bench.py for the roofline numbers): arm an
 * array of `capacity` hipEvent_t created by the caller; until dpr_stage_timing_end() every
 * raster / pullback call on THIS host thread records events[0] when it starts enqueuing
 * and the next event after each stage of its pipeline, on the call's stream.
 * dpr_stage_timing_end() disarms and returns the number of events recorded.
 * Stage order -- DPR_ALGO_ATOMIC raster: fill, splat; pullback: zero+grid_sum, gather.
 * DPR_ALGO_TILED, per pose -- raster: count, scan, scatter, tile_splat, halo;
 * pullback: count, scan, scatter, tile_gather, unpermute, pose_reduce.
 * DPR_ALGO_CHUNKED, 3-D grids -- raster: boxes, plan, own_splat, combine;
 * pullback: direct_gather, pose_reduce.
 * DPR_ALGO_CHUNKED, 2-D grids -- raster: sort, fill, chunk_splat;
 * pullback: sort, grid_sum, chunk_gather, reduce+unsort.
 * DPR_ALGO_ORDERED, per pose -- raster: keys, sort, ranges, gather; pullback (once): grid_sum, gather, reduce. */
int dpr_stage_timing_begin(void **events, int capacity);
int dpr_stage_timing_end(void);

/* Bytes of caller-provided device workspace needed by `op` with `algo`
 * (may be 0).  Returns (size_t)-1 on invalid arguments.  The workspace pointer must be
 * 256-byte aligned (DPR_ERR_WORKSPACE otherwise; hipMalloc / AMDGPU.jl / torch allocations
 * are); every non-NULL data pointer must be aligned to its element type
 * (DPR_ERR_INVALID_ARG otherwise, before any launch).  DPR_ALGO_TILED with a shape it would
 * refuse (a tile layer of more than 16384 tiles, P >= 2^32, KEEP / REUSE flags on a grid of more
 * than 32768 tiles) returns (size_t)-1 here too.
 * Contents and bounds (every dpr_workspace_bytes*_ex_* query of this header alike): the initial contents
 * of the workspace do not matter -- a long-lived buffer that other calls have written to serves as it is,
 * no clearing between calls; the library writes only inside [workspace, workspace + workspace_bytes), and
 * with a workspace_bytes equal to the query it uses no more; what a call leaves in the workspace is
 * unspecified, except what a KEEP forward leaves for its REUSE pullback. */
size_t dpr_workspace_bytes_f32(int op, int algo, int n_in, int n_out, const int64_t *grid,
                               int64_t P, int64_t B);
size_t dpr_workspace_bytes_f64(int op, int algo, int n_in, int n_out, const int64_t *grid,
                               int64_t P, int64_t B);
/* The same for a call that will pass `flags`: query with EXACTLY the flags of the call.
 * DPR_FLAG_MAX_POSE_GROUP and DPR_FLAG_COHERENT_POINTS change the layout (and the size) of the
 * tiled and the chunk-owner workspaces, and with DPR_ALGO_AUTO the KEEP / REUSE flags take part
 * in choosing the algorithm (see dpr_resolve_algo_ex).  A workspace that serves a KEEP raster
 * and its REUSE pullback is the larger of the two queries. */
size_t dpr_workspace_bytes_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                  const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                  const int64_t *grid, int64_t P, int64_t B);

/* Forward: out[.., b] = background[b] + sum_p splat(R[b] p + t[b]) * out_weight[b] * point_weight[p]
 * `out` is fully overwritten (src/raster.jl:27). */
int dpr_raster_f32(void *stream, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                   float *out, const float *points, const float *rotation,
                   const float *translation, const float *background, const float *out_weight,
                   const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_f64(void *stream, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                   double *out, const double *points, const double *rotation,
                   const double *translation, const double *background, const double *out_weight,
                   const double *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid, int64_t P,
                      int64_t B, float *out, const float *points, const float *rotation,
                      const float *translation, const float *background, const float *out_weight,
                      const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid, int64_t P,
                      int64_t B, double *out, const double *points, const double *rotation,
                      const double *translation, const double *background,
                      const double *out_weight, const double *point_weight, void *workspace,
                      size_t workspace_bytes);

/* Pullback.  All six outputs are OVERWRITTEN (ext/...CUDAExt.jl:272-276).
 * `background` is not an input of the arithmetic (src/raster_pullback.jl:7,78). */
int dpr_raster_pullback_f32(void *stream, int n_in, int n_out, const int64_t *grid, int64_t P,
                            int64_t B, const float *ds_dout, const float *points,
                            const float *rotation, const float *translation,
                            const float *out_weight, const float *point_weight, float *ds_dpoints,
                            float *ds_drotation, float *ds_dtranslation, float *ds_dbackground,
                            float *ds_dout_weight, float *ds_dpoint_weight, void *workspace,
                            size_t workspace_bytes);
int dpr_raster_pullback_f64(void *stream, int n_in, int n_out, const int64_t *grid, int64_t P,
                            int64_t B, const double *ds_dout, const double *points,
                            const double *rotation, const double *translation,
                            const double *out_weight, const double *point_weight,
                            double *ds_dpoints, double *ds_drotation, double *ds_dtranslation,
                            double *ds_dbackground, double *ds_dout_weight,
                            double *ds_dpoint_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                               int64_t P, int64_t B, const float *ds_dout, const float *points,
                               const float *rotation, const float *translation,
                               const float *out_weight, const float *point_weight,
                               float *ds_dpoints, float *ds_drotation, float *ds_dtranslation,
                               float *ds_dbackground, float *ds_dout_weight,
                               float *ds_dpoint_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                               int64_t P, int64_t B, const double *ds_dout, const double *points,
                               const double *rotation, const double *translation,
                               const double *out_weight, const double *point_weight,
                               double *ds_dpoints, double *ds_drotation, double *ds_dtranslation,
                               double *ds_dbackground, double *ds_dout_weight,
                               double *ds_dpoint_weight, void *workspace, size_t workspace_bytes);

/* Residual pullback: the caller one step out of raster_pullback!.
 * `out` is the result of dpr_raster_* for the same points / poses / weights, `target` a grid
 * of the same layout.  Computes, without materialising the sensitivity,
 *     ds_dout = residual_scale * (out - target)        README.md:151 (scale -2 there; +2 is
 *                                                      the gradient of examples/logo.jl:40-44)
 *     <all six outputs of dpr_raster_pullback_*>(ds_dout, ...)
 *     loss[b] = sum over pose b's grid of (out - target)^2      (loss may be NULL)
 * The sensitivity is formed in the kernels that consume it: the grid is read twice (out,
 * target) instead of read twice, written once and read again.  Flags as for
 * dpr_raster_pullback_ex_*; workspace: dpr_workspace_bytes_*(DPR_OP_RESIDUAL_PULLBACK, ...).  An explicit
 * DPR_ALGO_CHUNKED on a 3-D grid is refused (DPR_ERR_UNSUPPORTED_ALGO: the direct gather kernels have no
 * residual variant); DPR_ALGO_AUTO picks among the algorithms that have one. */
int dpr_raster_residual_pullback_f32(void *stream, int n_in, int n_out, const int64_t *grid,
                                     int64_t P, int64_t B, const float *out, const float *target,
                                     double residual_scale, const float *points,
                                     const float *rotation, const float *translation,
                                     const float *out_weight, const float *point_weight,
                                     float *loss, float *ds_dpoints, float *ds_drotation,
                                     float *ds_dtranslation, float *ds_dbackground,
                                     float *ds_dout_weight, float *ds_dpoint_weight,
                                     void *workspace, size_t workspace_bytes);
int dpr_raster_residual_pullback_f64(void *stream, int n_in, int n_out, const int64_t *grid,
                                     int64_t P, int64_t B, const double *out,
                                     const double *target, double residual_scale,
                                     const double *points, const double *rotation,
                                     const double *translation, const double *out_weight,
                                     const double *point_weight, double *loss, double *ds_dpoints,
                                     double *ds_drotation, double *ds_dtranslation,
                                     double *ds_dbackground, double *ds_dout_weight,
                                     double *ds_dpoint_weight, void *workspace,
                                     size_t workspace_bytes);
int dpr_raster_residual_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in,
                                        int n_out, const int64_t *grid, int64_t P, int64_t B,
                                        const float *out, const float *target,
                                        double residual_scale, const float *points,
                                        const float *rotation, const float *translation,
                                        const float *out_weight, const float *point_weight,
                                        float *loss, float *ds_dpoints, float *ds_drotation,
                                        float *ds_dtranslation, float *ds_dbackground,
                                        float *ds_dout_weight, float *ds_dpoint_weight,
                                        void *workspace, size_t workspace_bytes);
int dpr_raster_residual_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in,
                                        int n_out, const int64_t *grid, int64_t P, int64_t B,
                                        const double *out, const double *target,
                                        double residual_scale, const double *points,
                                        const double *rotation, const double *translation,
                                        const double *out_weight, const double *point_weight,
                                        double *loss, double *ds_dpoints, double *ds_drotation,
                                        double *ds_dtranslation, double *ds_dbackground,
                                        double *ds_dout_weight, double *ds_dpoint_weight,
                                        void *workspace, size_t workspace_bytes);

/* ---- MULTI-CHANNEL: C weights per point (1 <= C <= 16) ---------------------------------------
 * For channel c and pose b:
 *     out[i.., c, b] = background[c, b] + out_weight[b] * sum_p point_weight[c, p] * voxel_weight(i..; R_b p + t_b)
 * i.e. every plane is what dpr_raster_* returns for that channel's weights, and the gradients decompose
 * the same way: ds_dpoints, ds_drotation, ds_dtranslation, ds_dout_weight are the SUMS over c of the
 * single-channel results, ds_dpoint_weight[c, :] and ds_dbackground[c, b] the single-channel results of
 * channel c.  Layouts (column-major like the rest of this header):
 *   out, ds_dout                      (n_1, .., n_N, C, B): plane (c, b) is contiguous at (b * C + c) * G
 *                                     (memory of a contiguous NCHW / NCDHW (B, C, n_N, .., n_1) tensor)
 *   point_weight, ds_dpoint_weight    C x P, channel fastest (Vector{SVector{C,T}}, AoS like points); NULL => 1
 *   background, ds_dbackground        C x B; background NULL => 0
 *   out_weight                        B (one scalar per pose, shared by the channels); NULL => 1
 *   everything else                   as for dpr_raster_ex_* / dpr_raster_pullback_ex_*
 * Algorithms.  Forward: DPR_ALGO_ATOMIC for every (n_in, n_out) (the geometry of a (point, pose) is computed
 * once, C atomics per neighbour); DPR_ALGO_TILED for (2,2), (3,3), (3,2) on grids of at most 32768 tiles
 * (no slabs) with P < 2^32: every pose is binned ONCE, the scatter's slot map places the C weights
 * channel-planar in binned order, then one splat + halo pass per channel (no pose groups, no local binning
 * -- DPR_FLAG_COHERENT_POINTS is accepted and ignored).  Pullback: DPR_ALGO_ATOMIC (one gather pass serves
 * all channels).  AUTO (dpr_resolve_algo_channels): the forward takes DPR_ALGO_TILED where the single-channel
 * rule prefers DPR_ALGO_TILED for the shape (tiled_preferred: the point density per tile) and the channel
 * path supports it, DPR_ALGO_ATOMIC otherwise; the pullback always DPR_ALGO_ATOMIC.
 * Errors (status, message, nothing launched): C outside 1..16 and a NULL required pointer
 * DPR_ERR_INVALID_ARG; DPR_ALGO_CHUNKED, DPR_ALGO_TILED where unsupported (other dimension pairs, slabbed
 * grids, any pullback), the KEEP / REUSE flags and DPR_OP_RESIDUAL_PULLBACK DPR_ERR_UNSUPPORTED_ALGO.
 * DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning; DPR_FLAG_MAX_POSE_GROUP is accepted (the channel path
 * forms no pose groups).  Workspace: dpr_workspace_bytes_channels_ex_* with the call's op, algo and flags
 * ((size_t)-1 on invalid arguments; 0 for DPR_ALGO_ATOMIC; for DPR_ALGO_TILED at least the single-channel
 * DPR_ALGO_TILED workspace of the shape plus C * (P + 1) * sizeof(T)). */
int dpr_resolve_algo_channels(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                              int64_t C);
size_t dpr_workspace_bytes_channels_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                           const int64_t *grid, int64_t P, int64_t B, int64_t C);
size_t dpr_workspace_bytes_channels_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                           const int64_t *grid, int64_t P, int64_t B, int64_t C);
int dpr_raster_channels_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                               const int64_t *grid, int64_t P, int64_t B, int64_t C, float *out,
                               const float *points, const float *rotation, const float *translation,
                               const float *background, const float *out_weight,
                               const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_channels_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                               const int64_t *grid, int64_t P, int64_t B, int64_t C, double *out,
                               const double *points, const double *rotation,
                               const double *translation, const double *background,
                               const double *out_weight, const double *point_weight, void *workspace,
                               size_t workspace_bytes);
int dpr_raster_pullback_channels_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                        const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                        const float *ds_dout, const float *points,
                                        const float *rotation, const float *translation,
                                        const float *out_weight, const float *point_weight,
                                        float *ds_dpoints, float *ds_drotation,
                                        float *ds_dtranslation, float *ds_dbackground,
                                        float *ds_dout_weight, float *ds_dpoint_weight,
                                        void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_channels_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                        const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                        const double *ds_dout, const double *points,
                                        const double *rotation, const double *translation,
                                        const double *out_weight, const double *point_weight,
                                        double *ds_dpoints, double *ds_drotation,
                                        double *ds_dtranslation, double *ds_dbackground,
                                        double *ds_dout_weight, double *ds_dpoint_weight,
                                        void *workspace, size_t workspace_bytes);

/* ---- SAMPLING: N-linear interpolation of images at the transformed points ---------------------
 * The transpose of dpr_raster_* with respect to the point weights.  For pose b (R_b, t_b):
 *     values[p, b] = sum over the 2^N neighbours s that lie in the grid of
 *                    voxel_weight(deltas(R_b p + t_b), s) * image[ref(p, b) + shift_s, b]
 *     values[p, b] = 0 where the point is rejected (an axis with no in-range neighbour, NaN / Inf)
 * with exactly the cell choice, deltas, neighbour weights and drop rules of dpr_raster_* (the reference's
 * src/raster.jl:53-64, 85-108).  So
 *     sum_v (raster(pw) - background)[v, b] * image[v, b] = out_weight[b] * sum_p pw[p] * values[p, b]
 * and for B = 1 `values` is the ds_dpoint_weight of dpr_raster_pullback_* with ds_dout = image, out_weight = 1
 * and point_weight = 1.
 * The pullback takes ds_dvalues (P x B) and writes
 *   ds_dimage[.., b]     dpr_raster_* of pose b with point_weight = ds_dvalues[:, b], background 0, out_weight 1
 *   ds_dpoints           sum over b of the reference's point gradient (src/raster_pullback.jl:46-70) with
 *                        ds_dout = image_b, out_weight = 1, point_weight = ds_dvalues[:, b]
 *   ds_drotation[b], ds_dtranslation[b]   the per-pose sums of that same formula
 * (the reference's piecewise derivative of the interpolant, the one its pullback uses).
 * Layouts: values, ds_dvalues   P x B, point index fastest (pose b is the contiguous column at b * P);
 *          image, ds_dimage     (n_1, .., n_N, B) as `out` of dpr_raster_ex_*;
 *          everything else      as for dpr_raster_ex_* / dpr_raster_pullback_ex_*.
 * op: DPR_OP_RASTER (the forward) or DPR_OP_PULLBACK.  All 16 (n_in, n_out) with 1 <= n_in, n_out <= 4.
 * Outputs are overwritten, not accumulated.  Any pullback output may be NULL (not wanted); at least one must be
 * given; `image` may be NULL when only ds_dimage is wanted.
 * Algorithms.  Forward: DPR_ALGO_ATOMIC (= AUTO): one thread per point, the point in registers across a slice of
 * the poses, all 2^N gathers issued before the first use, the value stored coalesced, no atomics; workspace 0.
 * Pullback DPR_ALGO_ATOMIC: one fused kernel per (point, pose slice) forms from the same gathers the point
 * gradient, g * voxel_weight into ds_dimage (global float atomics) and the per-pose sums (wave -> block -> one
 * atomic per scalar per block); workspace 0.  Pullback DPR_ALGO_TILED, for (2,2), (3,3), (3,2): the same kernel
 * without the image atomics, then ds_dimage pose by pose from the tiled forward with B = 1, point_weight =
 * ds_dvalues[:, b], background and out_weight NULL -- each plane is what dpr_raster_ex_*(DPR_ALGO_TILED) returns
 * for those weights, and exactly as reproducible as that call (fp32: bit-identical where it sums exactly --
 * fixed point within its range guard, 3-D grids -- and at rounding level where it does not); workspace: that of
 * dpr_raster_ex_*(DPR_ALGO_TILED) for (grid, P, B = 1).  DPR_FLAG_COHERENT_POINTS is passed on to that forward;
 * the other flags except KEEP / REUSE are ignored.  AUTO (dpr_resolve_algo_sample): the pullback takes
 * DPR_ALGO_TILED where dpr_resolve_algo(DPR_OP_RASTER, .., P, 1) returns DPR_ALGO_TILED and the pair has it,
 * DPR_ALGO_ATOMIC otherwise.
 * Summation order.  values: over the neighbours s = 0 .. 2^N - 1 in order, as in dpr_raster_pullback_*.  Point
 * gradients: per pose in point_backward's order, summed over the poses of a slice in pose order, slices added
 * atomically.  Per-pose sums and the ATOMIC ds_dimage: global atomics, unordered.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): dimensions outside 1..4
 * DPR_ERR_UNSUPPORTED_DIMS; a bad op, a NULL required pointer or all outputs NULL DPR_ERR_INVALID_ARG;
 * DPR_ALGO_TILED for the forward or for another pair, DPR_ALGO_CHUNKED and the KEEP / REUSE flags
 * DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than dpr_workspace_bytes_sample_ex_* DPR_ERR_WORKSPACE.
 * dpr_workspace_bytes_sample_ex_* returns (size_t)-1 on invalid arguments. */
int dpr_resolve_algo_sample(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
int dpr_sample_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                      int64_t P, int64_t B, float *values, const float *image, const float *points,
                      const float *rotation, const float *translation, void *workspace,
                      size_t workspace_bytes);
int dpr_sample_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                      int64_t P, int64_t B, double *values, const double *image, const double *points,
                      const double *rotation, const double *translation, void *workspace,
                      size_t workspace_bytes);
int dpr_sample_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                               const int64_t *grid, int64_t P, int64_t B, const float *ds_dvalues,
                               const float *image, const float *points, const float *rotation,
                               const float *translation, float *ds_dimage, float *ds_dpoints,
                               float *ds_drotation, float *ds_dtranslation, void *workspace,
                               size_t workspace_bytes);
int dpr_sample_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                               const int64_t *grid, int64_t P, int64_t B, const double *ds_dvalues,
                               const double *image, const double *points, const double *rotation,
                               const double *translation, double *ds_dimage, double *ds_dpoints,
                               double *ds_drotation, double *ds_dtranslation, void *workspace,
                               size_t workspace_bytes);

/* ---- FORWARD-MODE DERIVATIVE: out_dot = J . v of dpr_raster_* for K = 1..16 tangents ------------------
 * For tangent k, pose b and point p, with coord = (R_b p + 1 + t_b) * n / 2 and (ref0, dlo) the cell and deltas
 * of dpr_raster_* (held FIXED: the one-sided derivative dpr_raster_pullback_* uses, so that J . v is the exact
 * transpose of the pullback for every input, points on cell faces included):
 *     cdot_n    = n_n / 2 * (sum_j Rdot_{k,b}[n, j] p_j + sum_j R_b[n, j] pdot_{k,p}[j] + tdot_{k,b}[n])
 *     a         = owdot_{k,b} * pw_p + ow_b * pwdot_{k,p}
 *     b_n       = ow_b * pw_p * cdot_n
 *     deposit_s = a * voxel_weight(dlo, s) + sum_n b_n * interp_weight(n, dlo, s)
 *     out_dot[cell, k, b] = bgdot_{k,b} + sum over (p, s) -> cell of deposit_s
 * interp_weight is the reference's piecewise derivative of the interpolant (src/raster_pullback.jl:150-160).
 * The drop rules are those of dpr_raster_*: a rejected point deposits nothing whatever its tangents hold (they
 * are not read), an out-of-range neighbour is dropped on its own.  out_weight / point_weight NULL = 1; the primal
 * background does not enter.
 * Layouts.  Every tangent holds K copies of its primal's layout, tangent k at k * (primal size): points_dot
 * K x P x n_in, rotation_dot K x B x (n_out x n_in column-major), translation_dot K x B x n_out,
 * point_weight_dot K x P; background_dot and out_weight_dot K x B (tangent k a contiguous run of B).  out_dot is
 * the channel layout with C = K: plane (k, b) at (b * K + k) * G.  Any tangent may be NULL (= zero; a NULL
 * tangent and a zero one give the same bits); with all of them NULL out_dot is zero-filled.  out_dot is
 * overwritten.  All 16 (n_in, n_out).
 * Algorithms.  DPR_ALGO_ATOMIC: background tangent fill, then one thread per point over a slice of the poses:
 * the cell, the 2^N voxel weights and the N * 2^N interpolation weights once per (point, pose), the K tangents a
 * run-time loop of 2^N global float atomics each; workspace 0.  DPR_ALGO_TILED, for (2,2), (3,3), (3,2) on grids
 * of one tile slab (at most 32768 tiles) and P < 2^32: each pose binned once (the per-pose binning of the
 * tiled channel forward), then per tangent one pass in binned order that writes the coefficients (a, b_n) of every
 * record, one LDS tile splat of the deposits and one halo pass with the background tangent fused into the
 * flush; workspace dpr_workspace_bytes_jvp_ex_* (independent of B and K).  AUTO (dpr_resolve_algo_jvp):
 * DPR_ALGO_TILED where the pair and the grid have it and dpr_resolve_algo(DPR_OP_RASTER, .., P, 1) returns
 * DPR_ALGO_TILED (the rule of the channel forward), DPR_ALGO_ATOMIC otherwise.  There is no DPR_ALGO_CHUNKED JVP.
 * Summation order and reproducibility.  ATOMIC: global float atomics, unordered (rounding level run to run).
 * TILED, fp32: 64-bit fixed-point sums per tile, exact, as the tiled forward -- a plane is bit-reproducible, and
 * the plane of tangent k of a K-tangent call is bit-identical to the K = 1 call on tangent k, except for tiles
 * split into parts (> max(4096, P / 256) records of one pose), whose parts add in fp32 and vary at rounding
 * level.  TILED, fp64: f64 LDS atomics, rounding level.  TILED and ATOMIC agree at rounding level.
 * Fixed-point guard.  |voxel_weight| <= 1 and |interp_weight| <= 1, so |deposit_s| <= m_p = |a| + sum_n |b_n|.
 * The scale and the 2^10 range guard of the tiled forward (PRECISION OF THE FIXED-POINT SUMS above) are taken per
 * scope -- one (pose, tangent) -- from the max / min non-zero m_p of its binned points; a scope whose m_p span
 * more than 2^10, or hold NaN / Inf, accumulates with f64 LDS atomics instead.
 * Errors (status, dpr_last_error text, nothing launched, out_dot untouched): dimensions outside 1..4
 * DPR_ERR_UNSUPPORTED_DIMS; K outside 1..16, a bad grid, NULL out_dot or a NULL primal (points with P > 0,
 * rotation, translation) DPR_ERR_INVALID_ARG; DPR_ALGO_TILED for another pair or an unsupported grid,
 * DPR_ALGO_CHUNKED and the KEEP / REUSE flags DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than
 * dpr_workspace_bytes_jvp_ex_* DPR_ERR_WORKSPACE.  The other flags are ignored.
 * dpr_workspace_bytes_jvp_ex_* returns (size_t)-1 on invalid arguments; dpr_resolve_algo_jvp a negative status. */
int dpr_resolve_algo_jvp(int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_jvp_ex_f32(int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                      int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_jvp_ex_f64(int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                      int64_t P, int64_t B, int64_t K);
int dpr_raster_jvp_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                          int64_t P, int64_t B, int64_t K, float *out_dot, const float *points,
                          const float *rotation, const float *translation, const float *out_weight,
                          const float *point_weight, const float *points_dot, const float *rotation_dot,
                          const float *translation_dot, const float *background_dot, const float *out_weight_dot,
                          const float *point_weight_dot, void *workspace, size_t workspace_bytes);
int dpr_raster_jvp_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                          int64_t P, int64_t B, int64_t K, double *out_dot, const double *points,
                          const double *rotation, const double *translation, const double *out_weight,
                          const double *point_weight, const double *points_dot, const double *rotation_dot,
                          const double *translation_dot, const double *background_dot,
                          const double *out_weight_dot, const double *point_weight_dot, void *workspace,
                          size_t workspace_bytes);

/* ---- PER-POSE CLOUDS: a different point cloud for every pose -------------------------------------------------
 * For pose b, with its own cloud points[b]:
 *     out[i.., b] = background[b] + out_weight[b] * sum_p point_weight[b, p] * voxel_weight(i..; R_b points[b, p] + t_b)
 * Plane b is exactly dpr_raster_* of (grid, points[b], R_b, t_b, background[b], out_weight[b], point_weight[b]):
 * the same cell choice, weights and drop rules.  The pullback decomposes the same way: ds_dpoints[b] and
 * ds_dpoint_weight[b] are the single-pose gradients of pose b -- disjoint across poses, no sum over poses -- and
 * the per-pose sums (ds_drotation, ds_dtranslation, ds_dbackground, ds_dout_weight) the single-pose ones.
 * Layouts (column-major like the rest of this header):
 *   points, ds_dpoints                 n_in x P x B: cloud b at b * P * n_in (a contiguous (B, P, n_in) tensor)
 *   point_weight, ds_dpoint_weight     P x B: cloud b's weights at b * P; point_weight NULL => 1
 *   everything else                    as for dpr_raster_ex_* / dpr_raster_pullback_ex_*
 * Clouds of different sizes: pad them to a common P with point_weight = 0.  A zero-weight point deposits nothing
 * and its ds_dpoints come back as 0 (its ds_dpoint_weight is the sensitivity of that weight, which a caller of
 * padded clouds drops); a point outside the grid gets 0 in both.  All six pullback outputs and `out` are overwritten.
 * op: DPR_OP_RASTER or DPR_OP_PULLBACK.  Flags: DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight
 * may then be NULL); DPR_FLAG_COHERENT_POINTS and DPR_FLAG_MAX_POSE_GROUP are accepted and ignored.
 * Algorithms.  DPR_ALGO_ATOMIC, all 16 (n_in, n_out): one thread per (point, pose) with global float atomics
 * (forward) or gathers (pullback; point gradients one plain store each, per-pose sums wave -> block -> one atomic
 * per block); workspace 0.  DPR_ALGO_TILED, (2,2), (3,3), (3,2): dpr_raster_ex_* / dpr_raster_pullback_ex_* with
 * DPR_ALGO_TILED and B = 1 on (cloud b, pose b), pose after pose on the stream; workspace: the single-pose tiled
 * one of (grid, P, 1), reused from pose to pose.  DPR_ALGO_CHUNKED, (2,2), (3,3), (3,2): pose-owned LDS tiles
 * (2-D 128 x 78 cells, 3-D 32 x 16 x 16); a workgroup owns (pose, tile, slice of consecutive points of the
 * pose's cloud), with as many slices as fill the device.  The forward deposits into its own tile only (fp32:
 * 64-bit fixed point with the scale and the 2^10 range guard of PRECISION OF THE FIXED-POINT SUMS taken per pose
 * from |out_weight[b]| * max |point_weight[b, :]|; fp64 and guarded poses: f64 LDS atomics) and flushes with
 * plain stores (one slice per (pose, tile)) or with float atomics onto the background (several); workspace
 * (fp32) 4 bytes per pose.  The pullback stages its tile of ds_dout (+ one halo cell on the high side); the tile
 * that holds a point's reference cell (-1 clamped to 0; tile 0 for a dropped point) writes its gradients;
 * per-pose sums go to one f64 partial per workgroup, reduced in a fixed order (ds_dbackground: k_grid_sum, one
 * float atomic per block); workspace 8 * (n_out * n_in + n_out + 1) * B * workgroups per pose bytes.  Every tile
 * re-reads its slices of the cloud.
 * AUTO (dpr_resolve_algo_clouds), from the shape alone: DPR_ALGO_CHUNKED where a pose's grid is at most 32 tiles
 * of DPR_ALGO_CHUNKED -- for the pullback only on 2-D grids of fp32 data; DPR_ALGO_TILED where
 * dpr_resolve_algo(op, .., P, 1) would choose it for one pose of the shape; DPR_ALGO_ATOMIC otherwise and for
 * every other pair.  dpr_resolve_algo_clouds answers for fp32 data: an fp64 pullback takes DPR_ALGO_ATOMIC where
 * it answers DPR_ALGO_CHUNKED.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): dimensions outside 1..4
 * DPR_ERR_UNSUPPORTED_DIMS; a bad op, negative P / B, a bad grid, a NULL required pointer, B * P * n_in beyond 2^60
 * DPR_ERR_INVALID_ARG; DPR_ALGO_TILED / DPR_ALGO_CHUNKED for another pair (or a grid the tiled path refuses), the
 * KEEP / REUSE flags and DPR_OP_RESIDUAL_PULLBACK DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than
 * dpr_workspace_bytes_clouds_ex_* DPR_ERR_WORKSPACE.  dpr_workspace_bytes_clouds_ex_* returns (size_t)-1 on
 * invalid arguments (0 for DPR_ALGO_ATOMIC); dpr_resolve_algo_clouds a negative status. */
int dpr_resolve_algo_clouds(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_clouds_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_clouds_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
int dpr_raster_clouds_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, float *out, const float *points, const float *rotation,
                             const float *translation, const float *background, const float *out_weight,
                             const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_clouds_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, double *out, const double *points, const double *rotation,
                             const double *translation, const double *background, const double *out_weight,
                             const double *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_clouds_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const float *ds_dout,
                                      const float *points, const float *rotation, const float *translation,
                                      const float *out_weight, const float *point_weight, float *ds_dpoints,
                                      float *ds_drotation, float *ds_dtranslation, float *ds_dbackground,
                                      float *ds_dout_weight, float *ds_dpoint_weight, void *workspace,
                                      size_t workspace_bytes);
int dpr_raster_pullback_clouds_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const double *ds_dout,
                                      const double *points, const double *rotation, const double *translation,
                                      const double *out_weight, const double *point_weight, double *ds_dpoints,
                                      double *ds_drotation, double *ds_dtranslation, double *ds_dbackground,
                                      double *ds_dout_weight, double *ds_dpoint_weight, void *workspace,
                                      size_t workspace_bytes);

/* ---- SMOOTH SPLAT: quadratic B-spline weights on 3^N cells, C1 in the point position ---------------------------
 * dpr_raster_* deposits a point with N-linear weights on 2^N cells: the image is continuous in the point position,
 * its gradient only piecewise constant per cell.  These entry points deposit with the next kernel order up, the
 * quadratic B-spline (particle-in-cell codes: TSC, triangular-shaped cloud): 3^N cells per point, weights that are
 * C1 in the position and sum to 1, so the pullback is continuous across cell boundaries and agrees with finite
 * differences everywhere.  Not in the reference.  Argument shapes, layouts, batching, defaults, background,
 * out_weight and point_weight are those of dpr_raster_ex_* / dpr_raster_pullback_ex_*; only the kernel differs.
 * For pose b and axis d of the output, with n_d cells (0-based cell j has its centre at j + 1/2):
 *     coord_d  = ((R_b p + t_b)_d + 1) * n_d / 2
 *     j0_d     = floor(coord_d)                 the cell whose centre is nearest
 *     u_d      = coord_d - (j0_d + 1/2)         in [-1/2, 1/2)
 *     w_d(-1)  = (1/2 - u_d)^2 / 2     w_d(0)  = 3/4 - u_d^2     w_d(+1)  = (1/2 + u_d)^2 / 2
 *     w'_d(-1) = -(1/2 - u_d)          w'_d(0) = -2 u_d          w'_d(+1) = 1/2 + u_d
 *     out[j0 + s, b] += out_weight[b] * point_weight[p] * prod_d w_d(s_d)        for s in {-1, 0, +1}^n_out
 * A point is accepted for a pose when -1 <= coord_d < n_d + 1 on every axis (tested in floating point before any
 * conversion to int; NaN / Inf are rejected).  Target cells outside the grid are dropped one by one, so mass is
 * lost only within 1.5 cells of the border.  `out` starts from background[b].
 * The pullback differentiates exactly this (no "cell held fixed": the function is C1).  Per point and pose,
 *     dcoord_k = ow * pw * sum_s g[j0 + s] * w'_k(s_k) * prod_{d != k} w_d(s_d),     scaled = dcoord * n / 2,
 *     ds_dtranslation += scaled,  ds_drotation += scaled * p^T,  ds_dpoints[p] += R^T * scaled,
 *     W = sum_s g[j0 + s] * prod_d w_d(s_d),  ds_dout_weight += W * pw,  ds_dpoint_weight[p] += W * ow,
 * and ds_dbackground[b] = sum(ds_dout[.., b]).  All six pullback outputs and `out` are overwritten.
 * (n_in, n_out): (2,2), (3,3) and (3,2); every other pair DPR_ERR_UNSUPPORTED_DIMS.
 * op: DPR_OP_RASTER or DPR_OP_PULLBACK (DPR_OP_RESIDUAL_PULLBACK: DPR_ERR_UNSUPPORTED_ALGO).  Flags:
 * DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight may then be NULL), KEEP / REUSE are refused
 * (DPR_ERR_UNSUPPORTED_ALGO), DPR_FLAG_COHERENT_POINTS and DPR_FLAG_MAX_POSE_GROUP are accepted and ignored.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  forward: one thread per point, pose loop inside, 3^N global float atomics per accepted
 *                    (point, pose).  Pullback: one thread per point, the poses looped inside the thread (sliced
 *                    exactly as dpr_raster_pullback_ex_* on DPR_ALGO_ATOMIC slices them, SUMMATION ORDER note 1),
 *                    the 3^N gathers issued one 3^(N-1) plane at a time, per-pose sums wave -> block -> one float
 *                    atomic per block, ds_dbackground one float atomic per block of cells.  Workspace 0: the
 *                    per-pose partials leave their block as atomics.
 *   DPR_ALGO_TILED   forward only (pullback: DPR_ERR_UNSUPPORTED_ALGO).  Per pose, the workspace reused: a 32-bit
 *                    key per point (the id of the tile that holds cell j0 clamped into the grid; all ones for a
 *                    rejected point), a stable radix sort of (key, point index) on the bits the tile count needs,
 *                    a start table over the tiles, then one workgroup per tile: it zeroes an LDS array of f64
 *                    cells over the tile plus one halo cell on both sides of every axis (3-D tiles 16 x 8 x 8,
 *                    2-D 64 x 16), adds every contribution of its run of points with f64 LDS atomics, and adds
 *                    each non-zero cell that lies inside the grid onto the background-filled `out` with one
 *                    global atomic in T, rows of axis 0 on consecutive lanes.  No global atomic per point; a
 *                    cell receives at most 3^N tile partials.  Workspace: 16 P bytes + the sort's temporary
 *                    storage + 4 (tiles + 1) bytes, every piece rounded up to 256, independent of B; 0 for P = 0.
 *                    LIMITS (DPR_ERR_UNSUPPORTED_ALGO, (size_t)-1 from the query): P <= 2^32 - 2 and fewer than
 *                    2^31 - 1 tiles.  COST: one workgroup owns a tile and adds its points 256 at a time, so the
 *                    forward's time grows with the most populated tile; a cloud packed into a few tiles runs at
 *                    the speed of those tiles (and many points on one cell serialise on its LDS atomic).
 * AUTO (dpr_resolve_algo_smooth), from the shape alone, never from the points: the pullback DPR_ALGO_ATOMIC; the
 * forward DPR_ALGO_TILED from 100 000 points on for a 3-D grid and from 500 000 for a 2-D grid (where the limits
 * above hold), DPR_ALGO_ATOMIC below (profiles/smooth_probe.txt: the tiled path pays a sort and four launches per
 * pose, the atomic one 3^N atomics per point).
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): as for the per-pose clouds --
 * a bad op, negative P / B, a bad grid, a NULL required pointer, a misaligned data pointer DPR_ERR_INVALID_ARG; a
 * workspace smaller than dpr_workspace_bytes_smooth_ex_* or not 256-byte aligned DPR_ERR_WORKSPACE.
 * dpr_workspace_bytes_smooth_ex_* returns (size_t)-1 for every refused combination; dpr_resolve_algo_smooth a
 * negative status. */
int dpr_resolve_algo_smooth(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_smooth_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_smooth_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B);
int dpr_raster_smooth_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, float *out, const float *points, const float *rotation,
                             const float *translation, const float *background, const float *out_weight,
                             const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_smooth_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, double *out, const double *points, const double *rotation,
                             const double *translation, const double *background, const double *out_weight,
                             const double *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_smooth_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const float *ds_dout,
                                      const float *points, const float *rotation, const float *translation,
                                      const float *out_weight, const float *point_weight, float *ds_dpoints,
                                      float *ds_drotation, float *ds_dtranslation, float *ds_dbackground,
                                      float *ds_dout_weight, float *ds_dpoint_weight, void *workspace,
                                      size_t workspace_bytes);
int dpr_raster_pullback_smooth_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const double *ds_dout,
                                      const double *points, const double *rotation, const double *translation,
                                      const double *out_weight, const double *point_weight, double *ds_dpoints,
                                      double *ds_drotation, double *ds_dtranslation, double *ds_dbackground,
                                      double *ds_dout_weight, double *ds_dpoint_weight, void *workspace,
                                      size_t workspace_bytes);

/* ---- SMOOTH SAMPLING: quadratic B-spline interpolation of images at the transformed points, C1 -----------------
 * The transpose of dpr_raster_smooth_* with respect to the point weights, as SAMPLING is of dpr_raster_*.  With
 * coord_d, j0_d, u_d, w_d and w'_d of SMOOTH SPLAT and its acceptance rule (-1 <= coord_d < n_d + 1 on every axis,
 * tested in floating point; NaN / Inf rejected), for pose b:
 *     values[p, b] = sum over s in {-1, 0, +1}^n_out with j0 + s inside the grid of
 *                    image[j0 + s, b] * prod_d w_d(s_d)
 *     values[p, b] = 0 for a rejected point
 * So
 *     sum_v (raster_smooth(pw) - background)[v, b] * image[v, b] = out_weight[b] * sum_p pw[p] * values[p, b],
 * for B = 1 `values` is the ds_dpoint_weight of dpr_raster_pullback_smooth_ex_* with ds_dout = image and
 * out_weight = 1, and a constant image samples to that constant wherever all 3^N cells are in the grid (coord_d in
 * [1, n_d - 1): the weights sum to 1).  `values` is C1 in the point position.
 * The pullback takes ds_dvalues (P x B) and writes
 *   ds_dimage[.., b]    dpr_raster_smooth_ex_* of pose b with point_weight = ds_dvalues[:, b], background 0,
 *                       out_weight 1
 *   and, with scaled_k = ds_dvalues[p, b] * n_k / 2 * sum_s image[j0 + s, b] * w'_k(s_k) * prod_{d != k} w_d(s_d),
 *   ds_dtranslation[b] = sum_p scaled,   ds_drotation[b] = sum_p scaled * p^T,   ds_dpoints[p] = sum_b R_b^T * scaled
 * -- the exact derivative; no cell is held fixed.
 * Layouts: values, ds_dvalues   P x B, point index fastest (pose b is the contiguous column at b * P);
 *          image, ds_dimage     (n_1, .., n_N, B) as `out` of dpr_raster_ex_*;
 *          everything else      as for dpr_sample_ex_* / dpr_sample_pullback_ex_*.
 * (n_in, n_out): (2,2), (3,3) and (3,2); every other pair DPR_ERR_UNSUPPORTED_DIMS.  op: DPR_OP_RASTER (the forward)
 * or DPR_OP_PULLBACK.  Outputs are overwritten, not accumulated.  Any pullback output may be NULL (not wanted, no
 * work done for it); at least one must be given; `image` may be NULL when only ds_dimage is wanted.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   Forward  DPR_ALGO_ATOMIC (= AUTO; DPR_ALGO_TILED: DPR_ERR_UNSUPPORTED_ALGO): one thread per point, the point in
 *            registers across a slice of the poses, the 3^N gathers issued one 3^(N-1) plane at a time, a dropped
 *            cell replaced by 0 with a select, the value stored coalesced; no atomics, workspace 0.
 *   Pullback DPR_ALGO_ATOMIC: one fused kernel per (point, pose slice), sliced as the smooth pullback slices the
 *            poses: from one set of gathers the point gradient (stored with one slice, added atomically with
 *            several) and the per-pose sums (wave -> block -> one atomic per scalar per block), and
 *            ds_dvalues * prod w into ds_dimage with global atomics; workspace 0.
 *   Pullback DPR_ALGO_TILED: the same kernel without the image atomics, then ds_dimage pose by pose: the planes
 *            zeroed, then the tiled smooth forward with B = 1, point_weight = ds_dvalues[:, b], out_weight NULL --
 *            plane b is what dpr_raster_smooth_ex_*(DPR_ALGO_TILED) returns for those weights.  Workspace: that of
 *            dpr_raster_smooth_ex_*(DPR_ALGO_TILED) for (grid, P), independent of B; its LIMITS and COST apply.
 * AUTO (dpr_resolve_algo_sample_smooth), from the shape alone: the forward DPR_ALGO_ATOMIC; the pullback
 * DPR_ALGO_TILED exactly where dpr_resolve_algo_smooth(DPR_OP_RASTER, .., P, 1) returns it, DPR_ALGO_ATOMIC
 * otherwise (that threshold was measured for the smooth forward; profiles/sample_smooth_probe.txt has this
 * pullback's own times on either path).
 * Flags: KEEP / REUSE are refused (DPR_ERR_UNSUPPORTED_ALGO), the others accepted and ignored.
 * Summation order.  values: plane by plane in smooth_point_backward's order, as the ds_dpoint_weight of the smooth
 * pullback.  Point gradients: summed over the poses of a slice in pose order, slices added atomically.  Per-pose
 * sums and ds_dimage: atomics, unordered.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): as for SMOOTH SPLAT; all outputs NULL
 * DPR_ERR_INVALID_ARG; a workspace smaller than dpr_workspace_bytes_sample_smooth_ex_* or not 256-byte aligned
 * DPR_ERR_WORKSPACE.  dpr_workspace_bytes_sample_smooth_ex_* returns (size_t)-1 for every refused combination;
 * dpr_resolve_algo_sample_smooth a negative status. */
int dpr_resolve_algo_sample_smooth(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_smooth_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_smooth_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B);
int dpr_sample_smooth_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, float *values, const float *image, const float *points,
                             const float *rotation, const float *translation, void *workspace,
                             size_t workspace_bytes);
int dpr_sample_smooth_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, double *values, const double *image, const double *points,
                             const double *rotation, const double *translation, void *workspace,
                             size_t workspace_bytes);
int dpr_sample_smooth_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const float *ds_dvalues,
                                      const float *image, const float *points, const float *rotation,
                                      const float *translation, float *ds_dimage, float *ds_dpoints,
                                      float *ds_drotation, float *ds_dtranslation, void *workspace,
                                      size_t workspace_bytes);
int dpr_sample_smooth_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, const double *ds_dvalues,
                                      const double *image, const double *points, const double *rotation,
                                      const double *translation, double *ds_dimage, double *ds_dpoints,
                                      double *ds_drotation, double *ds_dtranslation, void *workspace,
                                      size_t workspace_bytes);

/* ---- SMOOTH SPLAT, FORWARD MODE: out_dot = J . v of dpr_raster_smooth_* for K = 1..16 tangents -----------------
 * With coord_d, j0_d, u_d, w_d, w'_d and the acceptance rule of SMOOTH SPLAT (-1 <= coord_d < n_d + 1 on every axis,
 * tested in floating point; NaN / Inf rejected), for tangent k, pose b and accepted point p:
 *     cdot_n     = n_n / 2 * (sum_j Rdot_{k,b}[n, j] p_j + sum_j R_b[n, j] pdot_{k,p}[j] + tdot_{k,b}[n])
 *     a          = owdot_{k,b} * pw_p + ow_b * pwdot_{k,p}
 *     c          = ow_b * pw_p
 *     deposit(s) = a * prod_d w_d(s_d) + c * sum_n cdot_n * w'_n(s_n) * prod_{d != n} w_d(s_d),  s in {-1, 0, +1}^n_out
 *     out_dot[j0 + s, k, b] = bgdot_{k,b} + sum over (p, s) that land on the cell
 * Target cells outside the grid are dropped one by one.  No cell is held fixed: `out` is C1 in every input, so this
 * is the exact directional derivative, continuous across cell faces, and the exact transpose of
 * dpr_raster_pullback_smooth_ex_*.  A rejected point deposits nothing and none of its tangents is read (NaN there
 * leaves no trace).  out_weight / point_weight NULL = 1; the primal background does not enter.
 * Layouts, as dpr_raster_jvp_ex_*: every tangent holds K copies of its primal's layout, tangent k at
 * k * (primal size): points_dot K x P x n_in, rotation_dot K x B x (n_out x n_in column-major), translation_dot
 * K x B x n_out, point_weight_dot K x P, background_dot and out_weight_dot K x B.  out_dot is the channel layout
 * with C = K: plane (k, b) at (b * K + k) * G.  Any tangent may be NULL (= zero); with all of them NULL out_dot is
 * zero-filled.  out_dot is overwritten.  (n_in, n_out): (2,2), (3,3) and (3,2).
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  background tangent fill, then one thread per point, pose loop inside: the cell, the weights and
 *                    their derivatives once per accepted (point, pose), the K tangents a run-time loop of 3^N global
 *                    float atomics each.  Lanes of a wave that share a centre cell share all 3^N addresses: where a
 *                    wave holds runs of such lanes (a cloud with many points in a cell), up to four groups of equal
 *                    cells add their deposits across the wave in a fixed order first and issue one atomic per
 *                    (group, cell, tangent); every other lane issues its own.  Workspace 0.
 *   DPR_ALGO_TILED   background tangent fill, then per pose the key, sort and start table of
 *                    dpr_raster_smooth_ex_*(DPR_ALGO_TILED) ONCE -- they depend on the primal only -- and one launch
 *                    of (tiles x K) workgroups: workgroup (tile, k) adds the deposits of tangent k of the tile's run
 *                    of points into the LDS array of f64 cells (tile + halo) and adds every non-zero cell inside the
 *                    grid onto plane (k, b) with one global atomic in T.  Workspace: that of
 *                    dpr_raster_smooth_ex_*(DPR_ALGO_TILED) for (grid, P), independent of B and K; its LIMITS and
 *                    COST apply.
 * AUTO (dpr_resolve_algo_smooth_jvp), from the shape and K alone, never from the points: DPR_ALGO_TILED where
 * P * K >= 100 000 for a 3-D grid and P * K >= 400 000 for a 2-D grid (and the LIMITS hold), DPR_ALGO_ATOMIC
 * otherwise.  For K = 1 and a 3-D grid this is dpr_resolve_algo_smooth(DPR_OP_RASTER, .., P, 1), the rule this op
 * started from; that threshold was measured for the smooth forward, and this op's own times
 * (profiles/smooth_jvp_probe.txt, fp32, uniform clouds) moved it: the binning is paid once per pose whatever K, the
 * atomics K times, so 1e5 points x 16 poses -> 128^2 is 1.6x faster TILED at K = 4 and 4.4x at K = 12 although the
 * forward of that shape is faster ATOMIC.  Those two rows set the 2-D constant; between P * K = 1e5 and 4e5 nothing
 * was measured.
 * Summation order: the table in SUMMATION ORDER.  Both algorithms are at rounding level and agree at that level.
 * Flags: KEEP / REUSE are refused (DPR_ERR_UNSUPPORTED_ALGO), the others accepted and ignored.
 * P = 0 or B = 0: only the background tangent is written, DPR_OK.
 * Errors (status, dpr_last_error text, nothing launched, out_dot untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS; a bad grid, negative P / B, K outside 1..16, a NULL required pointer (out_dot, points
 * with P > 0, rotation, translation, grid), a misaligned data pointer DPR_ERR_INVALID_ARG; KEEP / REUSE,
 * DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm and DPR_ALGO_TILED outside its LIMITS
 * DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than dpr_workspace_bytes_smooth_jvp_ex_* or not 256-byte aligned
 * DPR_ERR_WORKSPACE.  dpr_workspace_bytes_smooth_jvp_ex_* returns (size_t)-1 for every refused combination;
 * dpr_resolve_algo_smooth_jvp a negative status. */
int dpr_resolve_algo_smooth_jvp(int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_smooth_jvp_ex_f32(int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                             int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_smooth_jvp_ex_f64(int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                             int64_t P, int64_t B, int64_t K);
int dpr_raster_smooth_jvp_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                 int64_t P, int64_t B, int64_t K, float *out_dot, const float *points,
                                 const float *rotation, const float *translation, const float *out_weight,
                                 const float *point_weight, const float *points_dot, const float *rotation_dot,
                                 const float *translation_dot, const float *background_dot,
                                 const float *out_weight_dot, const float *point_weight_dot, void *workspace,
                                 size_t workspace_bytes);
int dpr_raster_smooth_jvp_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                 int64_t P, int64_t B, int64_t K, double *out_dot, const double *points,
                                 const double *rotation, const double *translation, const double *out_weight,
                                 const double *point_weight, const double *points_dot, const double *rotation_dot,
                                 const double *translation_dot, const double *background_dot,
                                 const double *out_weight_dot, const double *point_weight_dot, void *workspace,
                                 size_t workspace_bytes);

/* ---- SMOOTH SPLAT, PER-POSE CLOUDS: the quadratic B-spline splat with a different cloud for every pose -------------
 * PER-POSE CLOUDS with the kernel of SMOOTH SPLAT.  For pose b, with its own cloud points[b]:
 *     out[i.., b] = background[b] + out_weight[b] * sum_p point_weight[b, p] * Bspline_weight(i..; R_b points[b, p] + t_b)
 * Plane b is dpr_raster_smooth_* of (grid, points[b], R_b, t_b, background[b], out_weight[b], point_weight[b]): the
 * same centre cell j0, the same weights on 3^N cells, the same acceptance -1 <= coord_d < n_d + 1, cells outside the
 * grid dropped one by one.  The pullback is its exact derivative and decomposes the same way: ds_dpoints[b] and
 * ds_dpoint_weight[b] are the single-pose smooth gradients of pose b -- disjoint across poses, no sum over poses --
 * and the four per-pose outputs the single-pose ones.  What a loop of B single-pose smooth calls computes, in one call.
 * Layouts: those of PER-POSE CLOUDS (points, ds_dpoints n_in x P x B, cloud b at b * P * n_in; point_weight,
 * ds_dpoint_weight P x B or NULL).  Clouds of different sizes: pad them to a common P with point_weight = 0; a
 * zero-weight point deposits nothing and gets ds_dpoints = 0.  All six pullback outputs and `out` are overwritten.
 * (n_in, n_out): (2,2), (3,3) and (3,2).  op: DPR_OP_RASTER or DPR_OP_PULLBACK.
 * Flags: DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight may then be NULL); DPR_FLAG_COHERENT_POINTS
 * is accepted and ignored; DPR_FLAG_MAX_POSE_GROUP(n) is HONOURED by the DPR_ALGO_TILED forward (below; pass the same
 * flags to the workspace query); KEEP / REUSE are refused.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  forward: one thread per (point, pose), a block inside one pose, 3^N global float atomics per
 *                    accepted (point, pose).  Pullback: one thread per (point, pose); the 3^N gathers one 3^(N-1)
 *                    plane at a time; ds_dpoints[b, p] and ds_dpoint_weight[b, p] one plain store each (no pose
 *                    slices, no accumulation); per-pose sums wave -> block -> one float atomic per scalar per
 *                    block; ds_dbackground one float atomic per block of cells.  Workspace 0.
 *   DPR_ALGO_TILED   forward only (pullback: DPR_ERR_UNSUPPORTED_ALGO).  The poses are binned in GROUPS of bg: for a
 *                    group, ONE key pass over its bg * P points (key = b_local * tiles + the tile of
 *                    dpr_raster_smooth_ex_*(DPR_ALGO_TILED), all ones for a rejected point; value = the flat index
 *                    b_local * P + p), ONE stable radix sort on the bits bg * tiles needs, ONE start table of
 *                    bg * tiles + 1 entries and ONE launch of bg * tiles workgroups, each the tile workgroup of
 *                    SMOOTH SPLAT for its (pose, tile): four launches per group instead of four per pose.
 *                    GROUP SIZE: bg is the largest number of poses <= B with bg * max(P, tiles) <= 2^24, at least 1,
 *                    and at most n under DPR_FLAG_MAX_POSE_GROUP(n), n in 1..16.  2^24 keeps every key below the
 *                    all-ones key and every flat index below 2^32 - 1 whenever bg > 1, and bounds the workspace
 *                    of a call at about 16 * 2^24 bytes of keys and indices plus the sort's storage (some 400 MB)
 *                    whatever B; nothing measured asked for another value (profiles/smooth_clouds_probe.txt).
 *                    With bg = 1 the LIMITS are those of SMOOTH SPLAT.  Workspace: that of
 *                    dpr_raster_smooth_ex_*(DPR_ALGO_TILED) evaluated for bg * tiles tiles and bg * P points, reused
 *                    from group to group; with a group of one exactly dpr_workspace_bytes_smooth_ex_*(DPR_OP_RASTER,
 *                    DPR_ALGO_TILED, .., P, 1); 0 for P = 0.  The COST note of SMOOTH SPLAT applies per (pose, tile).
 * AUTO (dpr_resolve_algo_smooth_clouds), from the shape alone, never from the points: the pullback DPR_ALGO_ATOMIC; the
 * forward DPR_ALGO_TILED where the default group holds bg * P >= 100 000 points for a 3-D grid and >= 400 000 for a
 * 2-D grid, a cloud holds at least 4 points per tile of the grid (P >= 4 * tiles) and the LIMITS hold;
 * DPR_ALGO_ATOMIC otherwise.  The first is the rule of dpr_resolve_algo_smooth applied to the group, because the
 * fixed cost is paid per group; this op's own times (profiles/smooth_clouds_probe.txt, fp32, uniform clouds) moved the
 * 2-D constant from 500 000 (3e4 points x 16 poses -> 128^2 is 1.27x faster TILED) and added the second condition
 * (1e4 x 16 -> 256^3, 0.6 points per tile, is 1.7x faster ATOMIC).  Between bg * P = 3.2e5 and 4.8e5 on 2-D grids and
 * between 1.8 and 4.9 points per tile nothing was measured; no 2-D row has fewer than 100 points per tile.
 * Summation order: the table in SUMMATION ORDER.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS (the grid is not looked at first); a bad op, negative P / B, a bad grid, a NULL required
 * pointer, a misaligned data pointer, B * P * n_in beyond 2^60 DPR_ERR_INVALID_ARG; DPR_OP_RESIDUAL_PULLBACK, KEEP /
 * REUSE, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm, a DPR_ALGO_TILED pullback and a DPR_ALGO_TILED
 * forward outside the LIMITS DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than
 * dpr_workspace_bytes_smooth_clouds_ex_* or not 256-byte aligned DPR_ERR_WORKSPACE.
 * dpr_workspace_bytes_smooth_clouds_ex_* returns (size_t)-1 for every refused combination;
 * dpr_resolve_algo_smooth_clouds a negative status. */
int dpr_resolve_algo_smooth_clouds(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_smooth_clouds_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_smooth_clouds_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B);
int dpr_raster_smooth_clouds_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B, float *out, const float *points,
                                    const float *rotation, const float *translation, const float *background,
                                    const float *out_weight, const float *point_weight, void *workspace,
                                    size_t workspace_bytes);
int dpr_raster_smooth_clouds_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B, double *out, const double *points,
                                    const double *rotation, const double *translation, const double *background,
                                    const double *out_weight, const double *point_weight, void *workspace,
                                    size_t workspace_bytes);
int dpr_raster_pullback_smooth_clouds_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, const float *ds_dout,
                                             const float *points, const float *rotation, const float *translation,
                                             const float *out_weight, const float *point_weight, float *ds_dpoints,
                                             float *ds_drotation, float *ds_dtranslation, float *ds_dbackground,
                                             float *ds_dout_weight, float *ds_dpoint_weight, void *workspace,
                                             size_t workspace_bytes);
int dpr_raster_pullback_smooth_clouds_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, const double *ds_dout,
                                             const double *points, const double *rotation,
                                             const double *translation, const double *out_weight,
                                             const double *point_weight, double *ds_dpoints, double *ds_drotation,
                                             double *ds_dtranslation, double *ds_dbackground,
                                             double *ds_dout_weight, double *ds_dpoint_weight, void *workspace,
                                             size_t workspace_bytes);

/* ---- SMOOTH SPLAT, MULTI-CHANNEL: the quadratic B-spline splat with C weights per point ---------------------------
 * MULTI-CHANNEL with the kernel of SMOOTH SPLAT.  For channel c and pose b:
 *     out[i.., c, b] = background[b, c] + out_weight[b] * sum_p point_weight[p, c] * Bspline_weight(i..; R_b p + t_b)
 * Plane (c, b) is dpr_raster_smooth_* of (grid, points, R_b, t_b, background[b, c], out_weight[b], point_weight[:, c]):
 * the same centre cell j0, the same weights on 3^N cells, the same acceptance -1 <= coord_d < n_d + 1, cells outside
 * the grid dropped one by one.  The cell, the weights and the offsets of a (point, pose) are computed once and serve
 * the C channels.  The pullback is the exact derivative (no cell is held fixed): ds_dpoints, ds_drotation,
 * ds_dtranslation and ds_dout_weight are the sums over c of the single-channel smooth gradients, ds_dpoint_weight[p, c]
 * and ds_dbackground[b, c] those of channel c.
 * Layouts: those of MULTI-CHANNEL.  point_weight, ds_dpoint_weight C x P (a point's C weights contiguous; point_weight
 * is REQUIRED: NULL with P > 0 is DPR_ERR_INVALID_ARG); background, ds_dbackground C x B (background may be NULL: 0);
 * out, ds_dout (n_1, .., n_N, C, B) column-major, plane (c, b) at (b * C + c) * G; out_weight one value per pose.
 * All six pullback outputs and `out` are overwritten.  C = 1..16; (n_in, n_out): (2,2), (3,3) and (3,2).
 * op: DPR_OP_RASTER or DPR_OP_PULLBACK.  P = 0: `out` is the backgrounds, the per-pose gradients are 0, ds_dbackground
 * the plane sums.  B = 0: DPR_OK after the checks, nothing is written.
 * Flags: DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight may then be NULL); DPR_FLAG_COHERENT_POINTS
 * and DPR_FLAG_MAX_POSE_GROUP are accepted and ignored; KEEP / REUSE are refused.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  forward: one thread per point, the pose loop inside; per accepted cell C global float atomics,
 *                    one into each plane.  Pullback: one thread per point, the poses sliced as SMOOTH SPLAT slices
 *                    them (SUMMATION ORDER note 1); per channel the 3^N gathers one 3^(N-1) plane at a time, all C
 *                    channels in one launch; per-pose sums wave -> block -> one float atomic per scalar per block;
 *                    ds_dbackground one float atomic per block of cells.  Workspace 0.
 *   DPR_ALGO_TILED   forward only (pullback: DPR_ERR_UNSUPPORTED_ALGO).  Per pose the key pass, the stable radix sort
 *                    and the start table of dpr_raster_smooth_ex_*(DPR_ALGO_TILED), ONCE for all C channels, then one
 *                    launch of tiles x ceil(C / 2) workgroups: a workgroup keeps the tile + halo of up to 2 channels
 *                    as f64 cells in LDS (3-D 28 800 bytes, 2-D 19 008), walks its run of the sorted points once and
 *                    adds every non-zero cell inside the grid onto its plane with one float atomic per (tile, cell,
 *                    channel).  LIMITS, COST and workspace: those of SMOOTH SPLAT --
 *                    dpr_workspace_bytes_smooth_ex_*(DPR_OP_RASTER, DPR_ALGO_TILED, .., P, 1) whatever B and C; 0 for
 *                    P = 0.
 * AUTO (dpr_resolve_algo_smooth_channels), from the shape and C alone, never from the points: the pullback
 * DPR_ALGO_ATOMIC; the forward DPR_ALGO_TILED where P * C >= 100 000 for a 3-D grid and >= 300 000 for a 2-D grid and
 * the LIMITS hold; DPR_ALGO_ATOMIC otherwise.  It is the rule of dpr_resolve_algo_smooth with P * C in the place of P:
 * the binning is paid once per pose, the atomics once per (point, channel).  This op's own times
 * (profiles/smooth_channels_probe.txt, fp32, uniform clouds, 18 rows) have DPR_ALGO_TILED ahead on every row, from
 * 1.29x (1e5 points x 16 poses -> 128^2, C = 3, P * C = 3e5: 1.48 against 1.90 ms) to 40x (1e7 -> 256^3, C = 16).
 * The 2-D constant lies between the smooth forward's row of that shape (P = 1e5, one weight: 0.68 ms ATOMIC against
 * 1.38 TILED, profiles/smooth_jvp_probe.txt) and this op's row at P * C = 3e5; the jvp rule's 4e5 would have lost
 * that row.  No row of this op lies below P * C = 3e5: the 3-D constant is the smooth forward's, not re-measured.
 * Summation order: the table in SUMMATION ORDER.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS (the grid is not looked at first); a bad op, negative P / B, a bad grid, C outside 1..16, a
 * NULL required pointer, a misaligned data pointer, an image beyond 2^62 cells DPR_ERR_INVALID_ARG;
 * DPR_OP_RESIDUAL_PULLBACK, KEEP / REUSE, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm, a DPR_ALGO_TILED
 * pullback and a DPR_ALGO_TILED forward outside the LIMITS DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than
 * dpr_workspace_bytes_smooth_channels_ex_* or not 256-byte aligned DPR_ERR_WORKSPACE.
 * dpr_workspace_bytes_smooth_channels_ex_* returns (size_t)-1 for every refused combination;
 * dpr_resolve_algo_smooth_channels a negative status. */
int dpr_resolve_algo_smooth_channels(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                                     int64_t C);
size_t dpr_workspace_bytes_smooth_channels_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                  const int64_t *grid, int64_t P, int64_t B, int64_t C);
size_t dpr_workspace_bytes_smooth_channels_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                  const int64_t *grid, int64_t P, int64_t B, int64_t C);
int dpr_raster_smooth_channels_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t C, float *out,
                                      const float *points, const float *rotation, const float *translation,
                                      const float *background, const float *out_weight, const float *point_weight,
                                      void *workspace, size_t workspace_bytes);
int dpr_raster_smooth_channels_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t C, double *out,
                                      const double *points, const double *rotation, const double *translation,
                                      const double *background, const double *out_weight, const double *point_weight,
                                      void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_smooth_channels_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                               const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                               const float *ds_dout, const float *points, const float *rotation,
                                               const float *translation, const float *out_weight,
                                               const float *point_weight, float *ds_dpoints, float *ds_drotation,
                                               float *ds_dtranslation, float *ds_dbackground, float *ds_dout_weight,
                                               float *ds_dpoint_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_smooth_channels_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                               const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                               const double *ds_dout, const double *points, const double *rotation,
                                               const double *translation, const double *out_weight,
                                               const double *point_weight, double *ds_dpoints, double *ds_drotation,
                                               double *ds_dtranslation, double *ds_dbackground, double *ds_dout_weight,
                                               double *ds_dpoint_weight, void *workspace, size_t workspace_bytes);

/* ---- RIGID BODIES: one cloud of K rigid bodies, a pose per (image, body) -------------------------------------------
 * Point p belongs to body[p] in [0, K) and is seen in image b through the pose of its body in that image:
 *     out[i.., b] = background[b]
 *                 + out_weight[b] * sum_p point_weight[p] * voxel_weight(i..; R[b, body[p]] points[p] + t[b, body[p]])
 * Cell choice, weights, drop rules and the fp operation order per (point, pose) are those of dpr_raster_*.  With
 * background 0, plane b is the sum over k of dpr_raster_* of the points with body[p] == k under pose (b, k), and
 * every gradient is the matching piece of dpr_raster_pullback_* of that subset: ds_dpoints[p] and
 * ds_dpoint_weight[p] sum over the images, ds_drotation[b, k] and ds_dtranslation[b, k] over the points of body k,
 * ds_dbackground[b] and ds_dout_weight[b] over all points.  The reference cell is held fixed, as everywhere.
 * Not in the reference.  It stands between dpr_raster_* (K = 1) and PER-POSE CLOUDS (every point free), which
 * would need the B warped copies of the cloud in memory.
 * Layouts (column-major like the rest of this header):
 *   points, point_weight, ds_dpoints, ds_dpoint_weight    as for dpr_raster_ex_* (one cloud, P points)
 *   body                        P values of int32_t (declared const void *; 4-byte aligned), read-only, no gradient
 *   rotation, ds_drotation      n_out x n_in x K x B: pose (b, k) at index b * K + k, each column-major
 *                               (a contiguous (B, K, n_in, n_out) tensor)
 *   translation, ds_dtranslation   n_out x K x B: pose (b, k) at (b * K + k) * n_out
 *   background, out_weight, ds_dbackground, ds_dout_weight    B values; out, ds_dout: grid x B
 * Dropped points.  A point whose body index lies outside [0, K) -- negative values included -- deposits nothing
 * and gets ds_dpoints = ds_dpoint_weight = 0, like a point outside the grid; the index is checked on the device,
 * lane by lane, before it addresses anything.  A body no accepted point belongs to gets gradients that are exactly
 * 0.  `out` and all six pullback outputs are overwritten.  P = 0 and B = 0 are valid: out = background, the
 * gradients are 0 (ds_dpoints and ds_dpoint_weight too when B = 0), ds_dbackground the grid sum.
 * (n_in, n_out): (2,2), (3,3), (3,2).  K >= 1 and B * K <= 2^31 - 1.
 * Algorithm: DPR_ALGO_ATOMIC (and AUTO, which resolves to it), workspace 0 -- dpr_workspace_bytes_bodies_ex_*
 * returns 0 for every accepted call and exists so that a later binned path changes no prototype.  Forward: one
 * thread per point, global float atomics, the images over grid.y.  Pullback: one thread per point with the image
 * loop inside; ds_dpoints / ds_dpoint_weight are plain stores when one launch covers all images and float atomics
 * onto zeroed buffers when the images are cut into slices (few points, many images), as in dpr_raster_pullback_*.
 * A wave whose points share one body -- SORT THE CLOUD BY BODY -- reads its pose with scalar loads and reduces its
 * pose sums wave -> block -> one float atomic per value; a wave with several bodies gathers its poses per lane and
 * reduces per body (masked wave sums over the lanes of each body in turn, one atomic per value and body).  Every
 * order is that of float atomics: results vary at rounding level from run to run.
 * Flags: DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight may then be NULL);
 * DPR_FLAG_COHERENT_POINTS is accepted and ignored.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS; a bad op, negative P / B, a bad grid, K < 1, B * K beyond 2^31 - 1, a NULL out, points,
 * body, rotation or translation while P * B > 0 (a NULL out or pullback output while B > 0), a misaligned data pointer
 * DPR_ERR_INVALID_ARG; any algorithm but AUTO / DPR_ALGO_ATOMIC, KEEP / REUSE, DPR_FLAG_MAX_POSE_GROUP and
 * DPR_OP_RESIDUAL_PULLBACK DPR_ERR_UNSUPPORTED_ALGO.  dpr_workspace_bytes_bodies_ex_* returns (size_t)-1 for every
 * refused combination; dpr_resolve_algo_bodies a negative status, DPR_ALGO_ATOMIC otherwise. */
int dpr_resolve_algo_bodies(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_bodies_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_bodies_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t *grid, int64_t P, int64_t B, int64_t K);
int dpr_raster_bodies_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, int64_t K, float *out, const float *points, const void *body,
                             const float *rotation, const float *translation, const float *background,
                             const float *out_weight, const float *point_weight, void *workspace,
                             size_t workspace_bytes);
int dpr_raster_bodies_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                             int64_t P, int64_t B, int64_t K, double *out, const double *points, const void *body,
                             const double *rotation, const double *translation, const double *background,
                             const double *out_weight, const double *point_weight, void *workspace,
                             size_t workspace_bytes);
int dpr_raster_pullback_bodies_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t K, const float *ds_dout,
                                      const float *points, const void *body, const float *rotation,
                                      const float *translation, const float *out_weight, const float *point_weight,
                                      float *ds_dpoints, float *ds_drotation, float *ds_dtranslation,
                                      float *ds_dbackground, float *ds_dout_weight, float *ds_dpoint_weight,
                                      void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_bodies_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t K, const double *ds_dout,
                                      const double *points, const void *body, const double *rotation,
                                      const double *translation, const double *out_weight,
                                      const double *point_weight, double *ds_dpoints, double *ds_drotation,
                                      double *ds_dtranslation, double *ds_dbackground, double *ds_dout_weight,
                                      double *ds_dpoint_weight, void *workspace, size_t workspace_bytes);

/* ---- SMOOTH SPLAT, RIGID BODIES: the quadratic B-spline splat of K rigid bodies, a pose per (image, body) ---------
 * RIGID BODIES with the kernel of SMOOTH SPLAT.  Point p belongs to body[p] in [0, K) and is seen in image b through
 * the pose of its body in that image:
 *     out[i.., b] = background[b]
 *                 + out_weight[b] * sum_p point_weight[p] * Bspline_weight(i..; R[b, body[p]] points[p] + t[b, body[p]])
 * Centre cell j0, the weights on 3^N cells, the acceptance -1 <= coord_d < n_d + 1, the cells outside the grid dropped
 * one by one and the fp operation order per (point, pose) are those of dpr_raster_smooth_*.  With background 0, plane
 * b is the sum over k of dpr_raster_smooth_* of the points with body[p] == k under pose (b, k), and every gradient is
 * the matching piece of dpr_raster_pullback_smooth_* of that subset: ds_dpoints[p] and ds_dpoint_weight[p] sum over the
 * images, ds_drotation[b, k] and ds_dtranslation[b, k] over the points of body k, ds_dbackground[b] and
 * ds_dout_weight[b] over all points.  The pullback is the exact derivative (the operator is C1, no cell is held fixed).
 * Not in the reference.  What a loop of K dpr_raster_smooth_* calls on subsets computes, or SMOOTH SPLAT, PER-POSE CLOUDS
 * on the B warped copies of the cloud, in one call and with the pose gradients.
 * Layouts: those of RIGID BODIES (body: P values of int32_t, declared const void *, 4-byte aligned; rotation,
 * ds_drotation n_out x n_in x K x B with pose (b, k) at index b * K + k; translation, ds_dtranslation n_out x K x B).
 * Dropped points.  A point whose body index lies outside [0, K) -- negative values included -- deposits nothing and
 * gets ds_dpoints = ds_dpoint_weight = 0; every kernel checks the index per lane before it addresses a pose.  A body no
 * accepted point belongs to gets gradients that are exactly 0.  `out` and all six pullback outputs are overwritten.
 * P = 0 and B = 0 are valid: out = background, the gradients are 0 (ds_dpoints and ds_dpoint_weight too when B = 0),
 * ds_dbackground the grid sum.  (n_in, n_out): (2,2), (3,3), (3,2).  K >= 1 and B * K <= 2^31 - 1.
 * op: DPR_OP_RASTER or DPR_OP_PULLBACK.
 * Flags: DPR_FLAG_NO_POINT_WEIGHT_GRAD keeps its meaning (ds_dpoint_weight may then be NULL); DPR_FLAG_COHERENT_POINTS
 * is accepted and ignored; DPR_FLAG_MAX_POSE_GROUP(n) is HONOURED by the DPR_ALGO_TILED forward (pass the same flags to
 * the workspace query), accepted and ignored by the DPR_ALGO_ATOMIC forward and REFUSED by the pullback, which forms no
 * groups; KEEP / REUSE are refused.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  forward: one thread per point, the images over grid.y, 3^N global float atomics per accepted
 *                    (point, image).  Pullback: one thread per point with the image loop inside, the images sliced as
 *                    SMOOTH SPLAT slices its poses (SUMMATION ORDER note 1); the 3^N gathers one 3^(N-1) plane at a
 *                    time.  A wave whose points share one body -- SORT THE CLOUD BY BODY -- reads its pose with scalar
 *                    loads and reduces its pose sums wave -> block -> one float atomic per value; a wave with several
 *                    bodies gathers its poses per lane and reduces per body (masked wave sums over the lanes of each
 *                    body in turn, one atomic per value and body).  With K = 1 and one image ds_dpoints and
 *                    ds_dpoint_weight are the bits of dpr_raster_pullback_smooth_ex_*(DPR_ALGO_ATOMIC).  Workspace 0.
 *   DPR_ALGO_TILED   forward only (pullback: DPR_ERR_UNSUPPORTED_ALGO).  The IMAGES are binned in groups of bg as
 *                    SMOOTH SPLAT, PER-POSE CLOUDS bins its poses: for a group, ONE key pass over its bg * P (point,
 *                    image) pairs (key = b_local * tiles + the tile of dpr_raster_smooth_ex_*(DPR_ALGO_TILED) under pose
 *                    (b, body[p]), all ones for a rejected point and for a body outside [0, K); value = the flat index
 *                    b_local * P + p), ONE stable radix sort, ONE start table of bg * tiles + 1 entries and ONE launch
 *                    of bg * tiles workgroups.  A workgroup walks the run of its (image, tile), takes p = value -
 *                    b_local * P, checks p and body[p] against their ranges (it does not trust the workspace),
 *                    gathers the pose of body[p] per lane, accumulates into the f64 LDS tile + halo of SMOOTH SPLAT and
 *                    adds every non-zero cell inside the grid with one float atomic per (tile, cell).  In a cloud
 *                    sorted by body a tile's run is contiguous per body (the sort is stable) and neighbouring lanes
 *                    gather the same pose.  GROUP SIZE, LIMITS and workspace: those of SMOOTH SPLAT, PER-POSE CLOUDS
 *                    for (P, B) -- bg the largest number of images <= B with bg * max(P, tiles) <= 2^24, at least 1,
 *                    at most n under DPR_FLAG_MAX_POSE_GROUP(n); the layout of dpr_raster_smooth_ex_*(DPR_ALGO_TILED)
 *                    for bg * tiles tiles and bg * P points, reused from group to group, whatever K; 0 for P = 0.
 *                    Every piece of the layout is written before it is read: keys and values by the key pass (all
 *                    bg * P entries), their sorted copies and the sort's storage by the sort, the start table by its
 *                    kernel.
 * AUTO (dpr_resolve_algo_smooth_bodies), from the shape alone, never from the points or `body`: the pullback
 * DPR_ALGO_ATOMIC; the forward DPR_ALGO_TILED where the default group holds bg * P >= 100 000 (point, image) pairs for a
 * 3-D grid and >= 160 000 for a 2-D grid, the cloud holds at least 4 points per tile of the grid (P >= 4 * tiles) and
 * the LIMITS hold; DPR_ALGO_ATOMIC otherwise.  K does not enter (the two forwards move by less than 10 % from K = 1 to
 * 64).  It is the rule of dpr_resolve_algo_smooth_clouds with this op's own times behind the constants
 * (profiles/smooth_bodies_probe.txt, tests/golden/smooth_bodies_auto.json; fp32, uniform clouds, 46 rows): they confirm
 * 100 000 (128^3: 1e4 points x 4 images a tie, 3e4 x 4 1.4x faster TILED) and the 4 points per tile (256^3: 1.8 per tile
 * 1.27x faster ATOMIC, 6.1 per tile 1.26x faster TILED) and move the 2-D constant from 400 000: DPR_ALGO_TILED is ahead
 * on every 2-D row measured, by 1.19x at the lowest (1e4 x 16 -> 128^2, bg * P = 160 000).  Below 160 000 on 2-D grids
 * and between 1.8 and 4.9 points per tile nothing was measured.  AUTO is within 1.15x of the faster forward on every row.
 * Summation order: the table in SUMMATION ORDER.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS (the grid is not looked at first); a bad op, negative P / B, a bad grid, K < 1, B * K beyond
 * 2^31 - 1, a NULL out, points, body, rotation or translation while P * B > 0 (a NULL out or pullback output while
 * B > 0), a misaligned data pointer DPR_ERR_INVALID_ARG; DPR_OP_RESIDUAL_PULLBACK, KEEP / REUSE,
 * DPR_FLAG_MAX_POSE_GROUP on the pullback, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm, a DPR_ALGO_TILED
 * pullback and a DPR_ALGO_TILED forward outside the LIMITS DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than
 * dpr_workspace_bytes_smooth_bodies_ex_* or not 256-byte aligned DPR_ERR_WORKSPACE.  Every refusal comes from one
 * check that the entry points, the query and the resolver share: dpr_workspace_bytes_smooth_bodies_ex_* returns
 * (size_t)-1 for every refused combination, dpr_resolve_algo_smooth_bodies a negative status. */
int dpr_resolve_algo_smooth_bodies(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                                   int64_t K);
size_t dpr_workspace_bytes_smooth_bodies_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_smooth_bodies_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t *grid, int64_t P, int64_t B, int64_t K);
int dpr_raster_smooth_bodies_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B, int64_t K, float *out,
                                    const float *points, const void *body, const float *rotation,
                                    const float *translation, const float *background, const float *out_weight,
                                    const float *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_smooth_bodies_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B, int64_t K, double *out,
                                    const double *points, const void *body, const double *rotation,
                                    const double *translation, const double *background, const double *out_weight,
                                    const double *point_weight, void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_smooth_bodies_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, int64_t K,
                                             const float *ds_dout, const float *points, const void *body,
                                             const float *rotation, const float *translation,
                                             const float *out_weight, const float *point_weight, float *ds_dpoints,
                                             float *ds_drotation, float *ds_dtranslation, float *ds_dbackground,
                                             float *ds_dout_weight, float *ds_dpoint_weight, void *workspace,
                                             size_t workspace_bytes);
int dpr_raster_pullback_smooth_bodies_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, int64_t K,
                                             const double *ds_dout, const double *points, const void *body,
                                             const double *rotation, const double *translation,
                                             const double *out_weight, const double *point_weight,
                                             double *ds_dpoints, double *ds_drotation, double *ds_dtranslation,
                                             double *ds_dbackground, double *ds_dout_weight,
                                             double *ds_dpoint_weight, void *workspace, size_t workspace_bytes);

/* ---- SMOOTH SPLAT, RIGID BODIES, FORWARD MODE: out_dot = J . v of dpr_raster_smooth_bodies_* for V = 1..16 tangents --
 * K is the number of bodies, V the number of tangents.  For image b, tangent v and an accepted point p with body
 * k = body[p] in [0, K), with coord_d, j0_d, u_d, w_d, w'_d of SMOOTH SPLAT under pose (b, k):
 *     cdot_n     = n_n / 2 * (sum_j Rdot_{v,b,k}[n, j] p_j + sum_j R_{b,k}[n, j] pdot_{v,p}[j] + tdot_{v,b,k}[n])
 *     a          = owdot_{v,b} * pw_p + ow_b * pwdot_{v,p}
 *     c          = ow_b * pw_p
 *     deposit(s) = a * prod_d w_d(s_d) + c * sum_n cdot_n * w'_n(s_n) * prod_{d != n} w_d(s_d),  s in {-1, 0, +1}^n_out
 *     out_dot[j0 + s, v, b] = bgdot_{v,b} + sum over (p, s) that land on the cell
 * No cell is held fixed: this is the exact directional derivative of dpr_raster_smooth_bodies_ex_* and the exact
 * transpose of dpr_raster_pullback_smooth_bodies_ex_*.  A point that dpr_raster_smooth_bodies_ex_* drops (outside the
 * acceptance range in that image, or body outside [0, K)) deposits nothing and none of its tangents is read: NaN
 * there leaves no trace.  Any tangent may be NULL (= zero, the same bits as an explicit zero); with all of them NULL
 * out_dot is zero-filled.  out_weight / point_weight NULL = 1; the primal background does not enter.
 * Layouts: the primals exactly as dpr_raster_smooth_bodies_ex_* (pose (b, k) at b * K + k, rotation column-major
 * n_out x n_in per pose, body int32_t).  Every tangent holds V copies of its primal's layout, tangent v first:
 * points_dot V x P x n_in; rotation_dot and translation_dot with pose tangent (v, b, k) at (v * B + b) * K + k;
 * out_weight_dot and background_dot at v * B + b; point_weight_dot at v * P + p.  out_dot is the channel layout with
 * C = V: plane (b, v) at (b * V + v) * G, as dpr_raster_smooth_jvp_ex_* has it.  out_dot is overwritten.
 * (n_in, n_out): (2,2), (3,3), (3,2).  K >= 1, B * K <= 2^31 - 1, V in 1..16.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   DPR_ALGO_ATOMIC  background tangent fill, then one thread per point, the images over grid.y: the primal pose as
 *                    the DPR_ALGO_ATOMIC forward of SMOOTH SPLAT, RIGID BODIES loads it, the cell, the weights and
 *                    their derivatives once per accepted (point, image), the V tangents a run-time loop of 3^N global
 *                    float atomics each.  The pose tangent of (v, b, body) is loaded as the primal pose is: scalar
 *                    loads where a wave's points share a body -- SORT THE CLOUD BY BODY -- a gather per lane
 *                    otherwise.  No lanes are combined before the atomics.  Workspace 0.
 *   DPR_ALGO_TILED   background tangent fill, then per GROUP of images the key pass, the stable sort and the start
 *                    table of the DPR_ALGO_TILED forward of SMOOTH SPLAT, RIGID BODIES ONCE -- they depend on the
 *                    primal only -- and ONE launch of (bg * tiles) x V workgroups: four launches per group, whatever V.
 *                    Workgroup (image, tile, v) walks the run of its (image, tile) with the forward's distrust of the
 *                    workspace (run clamped to the group's entries, point index to [0, P), body to [0, K)), gathers
 *                    pose and pose tangent per lane, adds the deposits of tangent v into the f64 LDS tile + halo and
 *                    adds every non-zero cell inside the grid onto plane (b, v) with one float atomic.  GROUP SIZE,
 *                    LIMITS and workspace: exactly those of dpr_raster_smooth_bodies_ex_*(DPR_ALGO_TILED) for the same
 *                    (grid, P, B, flags), independent of K and V; 0 for P = 0.  Every piece of the layout is written
 *                    before it is read, as there.
 * Flags: DPR_FLAG_MAX_POSE_GROUP(n) is HONOURED by DPR_ALGO_TILED (pass the same flags to the workspace query) and
 * ignored by DPR_ALGO_ATOMIC; KEEP / REUSE are refused; the others are accepted and ignored.
 * AUTO (dpr_resolve_algo_smooth_bodies_jvp), from the shape and V alone, never from the points or `body`:
 * DPR_ALGO_TILED where the default group holds bg * P * V^2 >= 96 000 for a 3-D grid and >= 160 000 for a 2-D grid, the
 * cloud holds at least 4 points per tile (P >= 4 * tiles) and the LIMITS hold; DPR_ALGO_ATOMIC otherwise.  K does not
 * enter.  For V = 1 this is the rule of dpr_resolve_algo_smooth_bodies(DPR_OP_RASTER) (with 96 000 for its 100 000).  The
 * rule started from that one with the group's work multiplied by V; this op's own times
 * (profiles/smooth_bodies_jvp_probe.txt, tests/golden/smooth_bodies_jvp_auto.json; fp32, uniform clouds, 140 rows, V = 1
 * and 12) left no constant for bg * P * V: 1000 points x 4 images -> 128^2 at V = 12 (4.8e4) is 1.28x faster TILED while 1e4 x
 * 8 at V = 1 (8e4) is 1.28x faster ATOMIC.  The binning is paid once per group whatever V and costs about one tangent's
 * atomics, so the group size from which DPR_ALGO_TILED pays falls faster than 1 / V: at V = 12 it is ahead on every row
 * measured with 4 points per tile (down to bg * P = 2 200), at V = 1 from the forward's constants on (2-D: 1e4 x 12
 * 1.14x faster ATOMIC, 1e4 x 16 level; 3-D: 24 000 x 4 -> 64^3 1.34x faster TILED, which moved 100 000 to 96 000).  With
 * V^2 AUTO is within 1.15x of the faster algorithm on every row (at most 1.06x behind).  Between V = 1 and V = 12
 * nothing was measured: there the square is an interpolation.
 * Summation order: both algorithms are at rounding level (float atomics in arrival order; DPR_ALGO_TILED adds a
 * tile's deposits in f64 first) and agree at that level.
 * P = 0: only the background tangent is written.  B = 0: nothing is done.  Both DPR_OK.
 * Errors (status, dpr_last_error text, nothing launched, out_dot untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS; a bad grid, negative P / B, K < 1, B * K beyond 2^31 - 1, V outside 1..16, a NULL out_dot
 * while B > 0, NULL points, body, rotation or translation while P * B > 0, a misaligned data pointer
 * DPR_ERR_INVALID_ARG; KEEP / REUSE, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm and DPR_ALGO_TILED
 * outside its LIMITS DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than dpr_workspace_bytes_smooth_bodies_jvp_ex_* or
 * not 256-byte aligned DPR_ERR_WORKSPACE.  Every refusal comes from one check that the entry points, the query and
 * the resolver share: the query returns (size_t)-1 for every refused combination, the resolver a negative status. */
int dpr_resolve_algo_smooth_bodies_jvp(int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B, int64_t K,
                                       int64_t V);
size_t dpr_workspace_bytes_smooth_bodies_jvp_ex_f32(int algo, unsigned flags, int n_in, int n_out,
                                                    const int64_t *grid, int64_t P, int64_t B, int64_t K, int64_t V);
size_t dpr_workspace_bytes_smooth_bodies_jvp_ex_f64(int algo, unsigned flags, int n_in, int n_out,
                                                    const int64_t *grid, int64_t P, int64_t B, int64_t K, int64_t V);
int dpr_raster_smooth_bodies_jvp_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                        const int64_t *grid, int64_t P, int64_t B, int64_t K, int64_t V,
                                        float *out_dot, const float *points, const void *body,
                                        const float *rotation, const float *translation, const float *out_weight,
                                        const float *point_weight, const float *points_dot,
                                        const float *rotation_dot, const float *translation_dot,
                                        const float *background_dot, const float *out_weight_dot,
                                        const float *point_weight_dot, void *workspace, size_t workspace_bytes);
int dpr_raster_smooth_bodies_jvp_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                        const int64_t *grid, int64_t P, int64_t B, int64_t K, int64_t V,
                                        double *out_dot, const double *points, const void *body,
                                        const double *rotation, const double *translation, const double *out_weight,
                                        const double *point_weight, const double *points_dot,
                                        const double *rotation_dot, const double *translation_dot,
                                        const double *background_dot, const double *out_weight_dot,
                                        const double *point_weight_dot, void *workspace, size_t workspace_bytes);

/* ---- SMOOTH SAMPLING, RIGID BODIES: quadratic B-spline interpolation of images at the points of K rigid bodies -------
 * SMOOTH SAMPLING through the poses of RIGID BODIES: the transpose of dpr_raster_smooth_bodies_* with respect to the
 * point weights, with one weight per (point, image).  Point p belongs to body[p] in [0, K) and is seen in image b
 * through pose b * K + body[p].  With coord_d, j0_d, u_d, w_d and w'_d of SMOOTH SPLAT under that pose and its
 * acceptance rule (-1 <= coord_d < n_d + 1 on every axis, tested in floating point; NaN / Inf rejected):
 *     values[p, b] = sum over s in {-1, 0, +1}^n_out with j0 + s inside the grid of
 *                    image[j0 + s, b] * prod_d w_d(s_d)
 *     values[p, b] = 0 for a point rejected in image b, or whose body lies outside [0, K)
 * So for every image b and every weight vector pw
 *     sum_v raster_smooth_bodies(pw; background 0, out_weight 1)[v, b] * image[v, b] = sum_p pw[p] * values[p, b],
 * and column b of `values` restricted to the points of body k is what dpr_sample_smooth_ex_* returns for that subset
 * under pose (b, k).  `values` is C1 in the points and in all B * K poses.  Not in the reference.
 * The pullback takes ds_dvalues (P x B) and writes
 *   ds_dimage[.., b]       dpr_raster_smooth_bodies_ex_* of image b alone with point_weight = ds_dvalues[:, b],
 *                          background 0 and out_weight 1
 *   and, with scaled_k = ds_dvalues[p, b] * n_k / 2 * sum_s image[j0 + s, b] * w'_k(s_k) * prod_{d != k} w_d(s_d)
 *   (that of SMOOTH SAMPLING, with ds_dout = image_b),
 *   ds_dtranslation[b, k]  sum of scaled over the points of body k
 *   ds_drotation[b, k]     sum of scaled * p^T over the same points
 *   ds_dpoints[p]          sum_b R[b, body[p]]^T * scaled
 * -- the exact derivative; no cell is held fixed.  A body without accepted points gets exact zeros; a dropped point
 * gets exact zero gradients and deposits nothing.
 * Layouts: values, ds_dvalues   P x B, point index fastest (image b is the contiguous column at b * P);
 *          image, ds_dimage     (n_1, .., n_N, B) as `out` of dpr_raster_ex_*;
 *          body                 P values of int32_t, declared const void *, 4-byte aligned;
 *          rotation, translation, ds_drotation, ds_dtranslation   those of RIGID BODIES (n_out x n_in x K x B and
 *                               n_out x K x B, pose (b, k) at index b * K + k; ds_drotation as
 *                               dpr_raster_pullback_bodies_ex_* writes it).
 * (n_in, n_out): (2,2), (3,3) and (3,2).  K >= 1 and B * K <= 2^31 - 1.  op: DPR_OP_RASTER (the forward) or
 * DPR_OP_PULLBACK.  Outputs are overwritten, not accumulated.  Any pullback output may be NULL (not wanted, no work
 * done for it); at least one must be given; `image` may be NULL when only ds_dimage is wanted.  P = 0 and B = 0 are
 * valid: nothing is sampled, the per-pose gradients and ds_dimage are 0 (ds_dpoints too when B = 0).
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED: DPR_ERR_UNSUPPORTED_ALGO).
 *   Forward  DPR_ALGO_ATOMIC (= AUTO; DPR_ALGO_TILED: DPR_ERR_UNSUPPORTED_ALGO): one thread per point, the point in
 *            registers across a slice of the images (sliced as SMOOTH SAMPLING slices its poses), the pose read with
 *            scalar loads where a wave's points share a body -- SORT THE CLOUD BY BODY -- and gathered per lane
 *            otherwise; the 3^N gathers one 3^(N-1) plane at a time; every values[p, b] stored coalesced, 0 for a
 *            dropped point.  No atomics and no sum across threads: values[p, b] has the same bits wherever the point
 *            stands in the cloud.  Workspace 0.
 *   Pullback DPR_ALGO_ATOMIC: one fused kernel per (point, image slice): from one set of gathers the point gradient
 *            (kept in registers across the images of a slice; stored with one slice, added atomically with several),
 *            the per-(image, body) sums, and ds_dvalues * prod w into ds_dimage with global float atomics.  The
 *            per-(image, body) sums of a block of 256 consecutive points: where its accepted points share one body,
 *            wave -> block -> one float atomic per value; otherwise every wave reduces per body (masked wave sums over
 *            the lanes of each body in turn) and, while K <= 64, adds these into a table of the block's bodies in LDS,
 *            from which ONE global atomic leaves per non-zero (body, value) of the block; with K > 64 one global
 *            atomic leaves per value, wave and body.  Workspace 0.
 *   Pullback DPR_ALGO_TILED: the same kernel without the image atomics, then ds_dimage: the planes zeroed and filled
 *            by GROUPS of images exactly as the DPR_ALGO_TILED forward of SMOOTH SPLAT, RIGID BODIES fills `out` -- its
 *            key pass, sort and start table per group, and one launch of bg * tiles workgroups on the f64 LDS tile +
 *            halo, which take the weight of the flat index b_local * P + p from ds_dvalues[(b0 + b_local) * P + p] and
 *            keep every check of that forward on the run, the point index and the body (the workspace contents are
 *            not trusted).  Plane b is what dpr_raster_smooth_bodies_ex_*(DPR_ALGO_TILED) returns for image b with
 *            those weights.  GROUP SIZE, LIMITS and workspace: those of
 *            dpr_workspace_bytes_smooth_bodies_ex_*(DPR_OP_RASTER, DPR_ALGO_TILED, flags, ..) for the same shape and
 *            DPR_FLAG_MAX_POSE_GROUP; 0 for P = 0.  The query cannot know whether ds_dimage is wanted and sizes for
 *            it; a call without ds_dimage reads no workspace.
 * AUTO (dpr_resolve_algo_sample_smooth_bodies), from the shape alone: the forward DPR_ALGO_ATOMIC; the pullback
 * DPR_ALGO_TILED exactly where dpr_resolve_algo_smooth_bodies(DPR_OP_RASTER, .., P, B, K) returns it, DPR_ALGO_ATOMIC
 * otherwise.  That rule was measured for the forward splat, not for this pullback.
 * Flags: KEEP / REUSE are refused; DPR_FLAG_MAX_POSE_GROUP(n) is HONOURED by the DPR_ALGO_TILED pullback (pass the same
 * flags to the workspace query) and REFUSED wherever the resolved algorithm is not the DPR_ALGO_TILED pullback, which
 * alone forms groups; the others are accepted and ignored.
 * Summation order.  values: plane by plane in the order of SMOOTH SAMPLING, no sum across threads.  Point gradients:
 * summed over the images of a slice in image order, slices added atomically.  Per-(image, body) sums and ds_dimage:
 * float atomics (LDS and global), unordered; DPR_ALGO_TILED adds a tile's deposits in f64 first.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS (the grid is not looked at first); a bad op, negative P / B, a bad grid, K < 1, B * K beyond
 * 2^31 - 1, all pullback outputs NULL, a NULL input that the call would read, a misaligned data pointer
 * DPR_ERR_INVALID_ARG; KEEP / REUSE, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm, a DPR_ALGO_TILED
 * forward, DPR_FLAG_MAX_POSE_GROUP as above and a DPR_ALGO_TILED pullback outside the LIMITS DPR_ERR_UNSUPPORTED_ALGO; a
 * workspace smaller than dpr_workspace_bytes_sample_smooth_bodies_ex_* (with ds_dimage wanted) or not 256-byte aligned
 * DPR_ERR_WORKSPACE.  Every refusal comes from one check that the entry points, the query and the resolver share:
 * dpr_workspace_bytes_sample_smooth_bodies_ex_* returns (size_t)-1 for every refused combination,
 * dpr_resolve_algo_sample_smooth_bodies a negative status. */
int dpr_resolve_algo_sample_smooth_bodies(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                                          int64_t K);
size_t dpr_workspace_bytes_sample_smooth_bodies_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                       const int64_t *grid, int64_t P, int64_t B, int64_t K);
size_t dpr_workspace_bytes_sample_smooth_bodies_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                       const int64_t *grid, int64_t P, int64_t B, int64_t K);
int dpr_sample_smooth_bodies_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                    int64_t P, int64_t B, int64_t K, float *values, const float *image,
                                    const float *points, const void *body, const float *rotation,
                                    const float *translation, void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_bodies_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                    int64_t P, int64_t B, int64_t K, double *values, const double *image,
                                    const double *points, const void *body, const double *rotation,
                                    const double *translation, void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_bodies_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, int64_t K,
                                             const float *ds_dvalues, const float *image, const float *points,
                                             const void *body, const float *rotation, const float *translation,
                                             float *ds_dimage, float *ds_dpoints, float *ds_drotation,
                                             float *ds_dtranslation, void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_bodies_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, int64_t K,
                                             const double *ds_dvalues, const double *image, const double *points,
                                             const void *body, const double *rotation, const double *translation,
                                             double *ds_dimage, double *ds_dpoints, double *ds_drotation,
                                             double *ds_dtranslation, void *workspace, size_t workspace_bytes);

/* ---- SMOOTH SAMPLING, MULTI-CHANNEL: quadratic B-spline interpolation of C-channel images at the points, C1 ----------
 * SMOOTH SAMPLING of the images SMOOTH SPLAT, MULTI-CHANNEL writes: C values per (point, pose), C = 1..16.  With coord_d,
 * j0_d, u_d, w_d and w'_d of SMOOTH SPLAT and its acceptance rule (-1 <= coord_d < n_d + 1 on every axis, tested in
 * floating point; NaN / Inf rejected; cells outside the grid dropped one by one), all from R_b p + t_b alone:
 *     values[p, c, b] = sum over s in {-1, 0, +1}^n_out with j0 + s inside the grid of
 *                       image[j0 + s, c, b] * prod_d w_d(s_d)
 *     values[p, c, b] = 0 for a rejected point
 * values[:, c, b] is dpr_sample_smooth_ex_* of plane (c, b), BIT FOR BIT in fp32 and fp64 (no atomics; every plane is
 * contracted in the same order).  The operator is the transpose of dpr_raster_smooth_channels_* in the point weights
 * with one weight per (point, channel, pose):
 *     sum_{v, c} ds_dimage[v, c, b] * image[v, c, b] = sum_{p, c} ds_dvalues[p, c, b] * values[p, c, b].
 * The pullback takes ds_dvalues and writes
 *   ds_dimage[.., c, b]  dpr_raster_smooth_ex_* of pose b with point_weight = ds_dvalues[:, c, b], background 0,
 *                        out_weight 1: pose b's C planes are dpr_raster_smooth_channels_ex_* with point_weight =
 *                        ds_dvalues[:, :, b]
 *   ds_dpoints, ds_drotation, ds_dtranslation
 *                        the sums over c of dpr_sample_smooth_pullback_ex_*'s gradients for plane (c, b) with
 *                        ds_dvalues[:, c, b]: scaled_k = n_k / 2 * sum_c ds_dvalues[p, c, b] * sum_s image[j0 + s, c, b]
 *                        * w'_k(s_k) * prod_{d != k} w_d(s_d), then as SMOOTH SAMPLING
 * -- the exact derivative; no cell is held fixed.
 * Layouts: image, ds_dimage     (n_1, .., n_N, C, B) as `out` of dpr_raster_smooth_channels_ex_*: plane (c, b) at
 *                               (b * C + c) * G;
 *          values, ds_dvalues   a point's C values contiguous, pose slowest: element (p, c, b) at (b * P + p) * C + c,
 *                               so that ds_dvalues + b * P * C is a point_weight of dpr_raster_smooth_channels_ex_*;
 *          everything else      as for dpr_sample_smooth_ex_* / dpr_sample_smooth_pullback_ex_*.
 * (n_in, n_out): (2,2), (3,3) and (3,2); every other pair DPR_ERR_UNSUPPORTED_DIMS.  op: DPR_OP_RASTER (the forward)
 * or DPR_OP_PULLBACK.  Outputs are overwritten, not accumulated.  Any pullback output may be NULL (not wanted, no
 * work done for it); at least one must be given; `image` may be NULL when only ds_dimage is wanted.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED, unknown ones: DPR_ERR_UNSUPPORTED_ALGO).
 *   Forward  DPR_ALGO_ATOMIC (= AUTO; DPR_ALGO_TILED: DPR_ERR_UNSUPPORTED_ALGO): one thread per point, the point in
 *            registers across a slice of the poses; the cell, the weights and the offsets once per (point, pose), then
 *            the planes in groups of four and a rest one by one; with C % 4 == 0, fp32 and `values` 16-byte aligned a
 *            group leaves as one 16-byte store; no atomics, workspace 0.
 *   Pullback DPR_ALGO_ATOMIC: one fused kernel per (point, pose slice), sliced as the smooth pullback slices the
 *            poses: per channel ds_dvalues * prod w into ds_dimage with C global atomics per accepted cell, and from
 *            the gathers of the C planes the n_out sums sum_c ds_dvalues * dcoord_c, which give the point gradient
 *            (stored with one slice, added atomically with several) and the per-pose sums (wave -> block -> one
 *            atomic per scalar per block); workspace 0.
 *   Pullback DPR_ALGO_TILED: the same kernel without the image atomics, then ds_dimage pose by pose: the planes
 *            zeroed, then the tiled smooth channel forward with B = 1, point_weight = ds_dvalues + b * P * C,
 *            out_weight NULL -- one binning per pose for all C channels; the C planes of pose b are what
 *            dpr_raster_smooth_channels_ex_*(DPR_ALGO_TILED) returns for those weights.  Workspace: that of
 *            dpr_raster_smooth_ex_*(DPR_ALGO_TILED) for (grid, P), independent of B and C; its LIMITS and COST apply.
 *            It is required only when ds_dimage is asked for and P, B > 0.
 * AUTO (dpr_resolve_algo_sample_smooth_channels), from the shape and C alone: the forward DPR_ALGO_ATOMIC; the pullback
 * DPR_ALGO_TILED exactly where dpr_resolve_algo_smooth_channels(DPR_OP_RASTER, .., P, 1, C) returns it, DPR_ALGO_ATOMIC
 * otherwise (that threshold was measured for the smooth channel forward; profiles/sample_smooth_channels_probe.txt
 * has this pullback's own times on either path).
 * Flags: KEEP / REUSE are refused (DPR_ERR_UNSUPPORTED_ALGO), the others accepted and ignored.
 * Workspace and stream: the contract of dpr_raster_ex_* holds -- the call only enqueues on `stream`, writes only
 * inside [workspace, workspace + workspace_bytes), and the initial contents of the workspace do not matter.
 * Summation order: the row of SUMMATION ORDER above.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS; C outside 1..16, a bad op, negative P / B, a bad grid, all pullback outputs NULL, a NULL
 * input that the call would read, a misaligned data pointer DPR_ERR_INVALID_ARG; KEEP / REUSE, DPR_ALGO_CHUNKED /
 * DPR_ALGO_ORDERED / an unknown algorithm, a DPR_ALGO_TILED forward and a DPR_ALGO_TILED pullback outside the LIMITS
 * DPR_ERR_UNSUPPORTED_ALGO; a workspace smaller than dpr_workspace_bytes_sample_smooth_channels_ex_* (with ds_dimage
 * wanted) or not 256-byte aligned DPR_ERR_WORKSPACE.  P = 0 or B = 0: DPR_OK, the outputs that still have elements
 * zeroed.  dpr_workspace_bytes_sample_smooth_channels_ex_* returns (size_t)-1 for every refused combination,
 * dpr_resolve_algo_sample_smooth_channels a negative status. */
int dpr_resolve_algo_sample_smooth_channels(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B,
                                            int64_t C);
size_t dpr_workspace_bytes_sample_smooth_channels_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                         const int64_t *grid, int64_t P, int64_t B, int64_t C);
size_t dpr_workspace_bytes_sample_smooth_channels_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                         const int64_t *grid, int64_t P, int64_t B, int64_t C);
int dpr_sample_smooth_channels_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t C, float *values,
                                      const float *image, const float *points, const float *rotation,
                                      const float *translation, void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_channels_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t *grid, int64_t P, int64_t B, int64_t C, double *values,
                                      const double *image, const double *points, const double *rotation,
                                      const double *translation, void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_channels_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                               const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                               const float *ds_dvalues, const float *image, const float *points,
                                               const float *rotation, const float *translation, float *ds_dimage,
                                               float *ds_dpoints, float *ds_drotation, float *ds_dtranslation,
                                               void *workspace, size_t workspace_bytes);
int dpr_sample_smooth_channels_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                               const int64_t *grid, int64_t P, int64_t B, int64_t C,
                                               const double *ds_dvalues, const double *image, const double *points,
                                               const double *rotation, const double *translation, double *ds_dimage,
                                               double *ds_dpoints, double *ds_drotation, double *ds_dtranslation,
                                               void *workspace, size_t workspace_bytes);

/* ---- SMOOTH SAMPLING, PER-POSE CLOUDS: quadratic B-spline interpolation of image b at cloud b, C1 ---------------------
 * SMOOTH SAMPLING with a different cloud for every pose: the transpose of dpr_raster_smooth_clouds_* with respect to
 * the point weights.  With coord_d, j0_d, u_d, w_d and w'_d of SMOOTH SPLAT and its acceptance rule (-1 <= coord_d <
 * n_d + 1 on every axis, tested in floating point; NaN / Inf rejected; cells outside the grid dropped one by one), all
 * from R_b points[b, p] + t_b:
 *     values[b, p] = sum over s in {-1, 0, +1}^n_out with j0 + s inside the grid of
 *                    image[j0 + s, b] * prod_d w_d(s_d)
 *     values[b, p] = 0 for a rejected point
 * Row b is dpr_sample_smooth_ex_* of (image[.., b], points[b], R_b, t_b) with B = 1, BIT FOR BIT in fp32 and fp64 (no
 * atomics, no sum across threads, the same order of operations).  What a loop of B single-pose smooth sampling calls
 * computes, in one call.  The adjoint identity, per pose:
 *     sum_v (raster_smooth_clouds(pw) - background)[v, b] * image[v, b] = out_weight[b] * sum_p pw[b, p] * values[b, p].
 * The pullback takes ds_dvalues (B, P) and writes
 *   ds_dimage[.., b]    dpr_raster_smooth_clouds_ex_* with point_weight = ds_dvalues, background 0, out_weight 1
 *   and, with scaled_k = ds_dvalues[b, p] * n_k / 2 * sum_s image[j0 + s, b] * w'_k(s_k) * prod_{d != k} w_d(s_d),
 *   ds_dtranslation[b] = sum_p scaled,   ds_drotation[b] = sum_p scaled * points[b, p]^T,
 *   ds_dpoints[b, p] = R_b^T * scaled  -- one pose per point, no sum over poses; 0 for a rejected point
 * -- the exact derivative; no cell is held fixed.  ds_dpoints[b] has the bits of the single-pose
 * dpr_sample_smooth_pullback_ex_*(DPR_ALGO_ATOMIC) for pose b.
 * Layouts: points, ds_dpoints   n_in x P x B as for PER-POSE CLOUDS: cloud b at b * P * n_in;
 *          values, ds_dvalues   (B, P) contiguous, point index fastest: row b at b * P -- the layout of point_weight of
 *                               dpr_raster_smooth_clouds_ex_*.  (Not the P x B of SMOOTH SAMPLING read as a transpose:
 *                               the memory is the same, the pose is the slow index in both.)
 *          image, ds_dimage     (n_1, .., n_N, B) as `out` of dpr_raster_ex_*;
 *          ds_drotation         n_out x n_in column-major per pose;  ds_dtranslation  n_out per pose.
 * Clouds of different sizes: pad them to a common P.  The values of the padded points are to be ignored and their
 * ds_dvalues set to 0: such a point gets ds_dpoints = 0, adds nothing to the pose gradients and deposits nothing.
 * (n_in, n_out): (2,2), (3,3) and (3,2); every other pair DPR_ERR_UNSUPPORTED_DIMS.  op: DPR_OP_RASTER (the forward)
 * or DPR_OP_PULLBACK.  Outputs are overwritten, not accumulated.  Any pullback output may be NULL (not wanted, no
 * work done for it); at least one must be given; `image` may be NULL when only ds_dimage is wanted.
 * Algorithms (DPR_ALGO_CHUNKED, DPR_ALGO_ORDERED, unknown ones: DPR_ERR_UNSUPPORTED_ALGO).
 *   Forward  DPR_ALGO_ATOMIC (= AUTO; DPR_ALGO_TILED: DPR_ERR_UNSUPPORTED_ALGO): one thread per (point, pose), a block
 *            inside one pose, the poses strided over at most 65 535 rows of blocks; the 3^N gathers issued one
 *            3^(N-1) plane at a time, a dropped cell replaced by 0 with a select; every value stored coalesced; no
 *            atomics, workspace 0.
 *   Pullback DPR_ALGO_ATOMIC: one fused kernel, one thread per (point, pose): from one set of gathers the point
 *            gradient (one plain store) and the per-pose sums (wave -> block -> one atomic per scalar per block), and
 *            ds_dvalues * prod w into ds_dimage with 3^N global atomics; workspace 0.
 *   Pullback DPR_ALGO_TILED: the same kernel without the image atomics, then ds_dimage: the planes zeroed, then the
 *            tiled forward of SMOOTH SPLAT, PER-POSE CLOUDS with point_weight = ds_dvalues and out_weight NULL, the
 *            poses binned in its GROUPS -- the planes are what dpr_raster_smooth_clouds_ex_*(DPR_ALGO_TILED) adds for
 *            those weights.  GROUP SIZE, LIMITS and COST: those of SMOOTH SPLAT, PER-POSE CLOUDS.  Workspace:
 *            dpr_workspace_bytes_smooth_clouds_ex_*(DPR_OP_RASTER, DPR_ALGO_TILED, flags, ..) for the same shape and
 *            flags; it is required only when ds_dimage is asked for and P, B > 0.
 * AUTO (dpr_resolve_algo_sample_smooth_clouds), from the shape alone: the forward DPR_ALGO_ATOMIC; the pullback
 * DPR_ALGO_TILED exactly where dpr_resolve_algo_smooth_clouds(DPR_OP_RASTER, ..) returns it, DPR_ALGO_ATOMIC otherwise
 * (that rule was measured for the splat; profiles/sample_smooth_clouds_probe.txt has this pullback's own times on
 * either path and names the rows where the rule picks the slower one).
 * Flags: DPR_FLAG_MAX_POSE_GROUP(n) is HONOURED by the DPR_ALGO_TILED pullback (pass the same flags to the workspace
 * query) and ignored elsewhere; KEEP / REUSE are refused (DPR_ERR_UNSUPPORTED_ALGO); the others accepted and ignored.
 * Workspace and stream: the contract of dpr_raster_ex_* holds -- the call only enqueues on `stream`, writes only
 * inside [workspace, workspace + workspace_bytes), and the initial contents of the workspace do not matter.
 * Summation order.  values and ds_dpoints: no sum across threads -- plane by plane in smooth_point_backward's order, as
 * SMOOTH SAMPLING; reproducible bit for bit.  Per-pose sums: lanes of a wave, waves of a block, then one atomic per
 * block: unordered across blocks.  ds_dimage: DPR_ALGO_ATOMIC global atomics, unordered; DPR_ALGO_TILED the order of
 * the tiled forward of SMOOTH SPLAT, PER-POSE CLOUDS (f64 cells in LDS, then at most 3^N tile partials per cell), which
 * depends on the group size.
 * Errors (status, dpr_last_error text, nothing launched, outputs untouched): a pair outside the three
 * DPR_ERR_UNSUPPORTED_DIMS (the grid is not looked at first); a bad op, negative P / B, a bad grid, B * P * n_in beyond
 * 2^60 or G * B beyond 2^62, all pullback outputs NULL, a NULL input that the call would read, a misaligned data
 * pointer DPR_ERR_INVALID_ARG; KEEP / REUSE, DPR_ALGO_CHUNKED / DPR_ALGO_ORDERED / an unknown algorithm, a
 * DPR_ALGO_TILED forward and a DPR_ALGO_TILED pullback outside the LIMITS DPR_ERR_UNSUPPORTED_ALGO; a workspace
 * smaller than dpr_workspace_bytes_sample_smooth_clouds_ex_* (with ds_dimage wanted) or not 256-byte aligned
 * DPR_ERR_WORKSPACE.  P = 0 or B = 0: DPR_OK, the outputs that still have elements zeroed.
 * dpr_workspace_bytes_sample_smooth_clouds_ex_* returns (size_t)-1 for every refused combination,
 * dpr_resolve_algo_sample_smooth_clouds a negative status. */
int dpr_resolve_algo_sample_smooth_clouds(int op, int n_in, int n_out, const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_smooth_clouds_ex_f32(int op, int algo, unsigned flags, int n_in, int n_out,
                                                       const int64_t *grid, int64_t P, int64_t B);
size_t dpr_workspace_bytes_sample_smooth_clouds_ex_f64(int op, int algo, unsigned flags, int n_in, int n_out,
                                                       const int64_t *grid, int64_t P, int64_t B);
int dpr_sample_smooth_clouds_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                    int64_t P, int64_t B, float *values, const float *image, const float *points,
                                    const float *rotation, const float *translation, void *workspace,
                                    size_t workspace_bytes);
int dpr_sample_smooth_clouds_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out, const int64_t *grid,
                                    int64_t P, int64_t B, double *values, const double *image, const double *points,
                                    const double *rotation, const double *translation, void *workspace,
                                    size_t workspace_bytes);
int dpr_sample_smooth_clouds_pullback_ex_f32(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, const float *ds_dvalues,
                                             const float *image, const float *points, const float *rotation,
                                             const float *translation, float *ds_dimage, float *ds_dpoints,
                                             float *ds_drotation, float *ds_dtranslation, void *workspace,
                                             size_t workspace_bytes);
int dpr_sample_smooth_clouds_pullback_ex_f64(void *stream, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t *grid, int64_t P, int64_t B, const double *ds_dvalues,
                                             const double *image, const double *points, const double *rotation,
                                             const double *translation, double *ds_dimage, double *ds_dpoints,
                                             double *ds_drotation, double *ds_dtranslation, void *workspace,
                                             size_t workspace_bytes);

/* Pose-independent spatial pre-sort of the model-frame points along a Hilbert curve (any run
 * of consecutive sorted points is a compact blob; 3-D: 30-bit keys, 1024^3 cells over [-1, 1)^3) --
 * not in the reference; every algorithm here is faster on coherent input and the sort only depends
 * on the points.  points_sorted[i] = points[perm[i]] (and point weights likewise; pass NULL for
 * both weight pointers when unused).  Gradients of the sorted cloud go back with
 * ds_dpoints[perm[i]] = ds_dpoints_sorted[i].  n_in = 2 or 3; P < 2^32. */
size_t dpr_sort_points_workspace_bytes(int64_t P);
int dpr_sort_points_f32(void *stream, int n_in, int64_t P, const float *points,
                        float *points_sorted, uint32_t *perm, const float *point_weight,
                        float *point_weight_sorted, void *workspace, size_t workspace_bytes);
int dpr_sort_points_f64(void *stream, int n_in, int64_t P, const double *points,
                        double *points_sorted, uint32_t *perm, const double *point_weight,
                        double *point_weight_sorted, void *workspace, size_t workspace_bytes);

/* ---- multi-GPU: pose sharding over RCCL (one process or task per GPU) ------------------------
 * The batched pullback shards over poses: rank r owns the contiguous pose block
 * dpr_shard_range(B, r, world), the points are replicated, every per-pose output is disjoint and
 * the point gradients sum over ranks with ONE all-reduce -- the multi-process form of the
 * reference's per-thread slabs + sum (src/raster_pullback.jl:112-147).  The forward needs no
 * exchange: call dpr_raster_* on the local pose block.
 *
 *   rank 0:  dpr_comm_unique_id(id, DPR_COMM_ID_BYTES); ship the 128 bytes to the other ranks by
 *            the host's own means (MPI, a file, Julia Distributed); every rank, with its GPU
 *            current: dpr_comm_init(&comm, world, rank, id); ... ; dpr_comm_destroy(comm).
 * RCCL is loaded at run time (librccl.so.1); DPR_ERR_HIP if it is not available. */
#define DPR_COMM_ID_BYTES 128
typedef struct dpr_comm dpr_comm_t;
int dpr_comm_unique_id(void *id_out, size_t id_bytes);
int dpr_comm_init(dpr_comm_t **comm_out, int world, int rank, const void *id);
int dpr_comm_destroy(dpr_comm_t *comm);
int dpr_comm_world(const dpr_comm_t *comm);
int dpr_comm_rank(const dpr_comm_t *comm);
void dpr_shard_range(int64_t batch, int rank, int world, int64_t *lo, int64_t *hi);
/* dpr_raster_pullback_<T> on this rank's B_local poses (all `_local` arguments are the rank's
 * slices), then all-reduce(sum) of ds_dpoints / ds_dpoint_weight over the communicator on
 * `stream`: after the call they hold the global sums on every rank.  One all-reduce when the two
 * buffers are adjacent (ds_dpoint_weight == ds_dpoints + n_in * P), a grouped pair otherwise.
 *
 * When the LOCAL pullback of a rank fails (non-zero status, e.g. a workspace sized for another
 * rank's B_local) the rank still JOINS the all-reduce, with its two gradient buffers filled with
 * NaN, and returns its own error afterwards: no peer is left blocked in the collective, and every
 * rank sees NaN point gradients instead of sums that silently miss one rank's poses.  Only a rank
 * whose gradient buffers are NULL cannot take part; its error text says so, and the communicator
 * must then be destroyed on every rank (the peers are blocked).  dpr_shard_range with an invalid
 * (rank, world) yields the empty range [0, 0). */
int dpr_raster_pullback_sharded_f32(dpr_comm_t *comm, void *stream, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B_local,
                                    const float *ds_dout_local, const float *points,
                                    const float *rotation_local, const float *translation_local,
                                    const float *out_weight_local, const float *point_weight,
                                    float *ds_dpoints, float *ds_drotation_local,
                                    float *ds_dtranslation_local, float *ds_dbackground_local,
                                    float *ds_dout_weight_local, float *ds_dpoint_weight,
                                    void *workspace, size_t workspace_bytes);
int dpr_raster_pullback_sharded_f64(dpr_comm_t *comm, void *stream, int n_in, int n_out,
                                    const int64_t *grid, int64_t P, int64_t B_local,
                                    const double *ds_dout_local, const double *points,
                                    const double *rotation_local, const double *translation_local,
                                    const double *out_weight_local, const double *point_weight,
                                    double *ds_dpoints, double *ds_drotation_local,
                                    double *ds_dtranslation_local, double *ds_dbackground_local,
                                    double *ds_dout_weight_local, double *ds_dpoint_weight,
                                    void *workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DPR_H */
