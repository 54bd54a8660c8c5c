// DPR_ALGO_TILED / DPR_ALGO_CHUNKED entry points shared between the API layer (dpr_api.hip and the
// dpr_api_*.hip of the op families), dpr_tiled.hip, dpr_owner.hip, dpr_chunkown.hip and dpr_sort.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dpr_device.h"
#include "dpr_jvp.h"

namespace dpr {

int fail(int code, const char* fmt, ...);

// returns DPR_ERR_HIP (message recorded) from the calling function if a HIP call fails
#define DPR_HIP(expr)                                                                \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess)                                                        \
            return fail(DPR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// n of DPR_FLAG_MAX_POSE_GROUP(n) (include/dpr.h: bits 8 .. 15 of the flags; 0: the library's limit)
inline int max_pose_group(unsigned flags) { return (int)((flags >> 8) & 0xffu); }

// workspace pieces start on 256-byte boundaries
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

template <int NO> GridDesc<NO> make_grid_desc(const int64_t* grid, int64_t G) {
    GridDesc<NO> gd;
    for (int d = 0; d < NO; ++d) gd.n[d] = (int)grid[d];
    gd.G = G;
    return gd;
}

// records hipEvent k (if stage timing is armed, see dpr_stage_timing_begin) on `st`
void stage_mark(hipStream_t st);

// `bytes` bytes at `p` become zero, by a kernel on `st` (dpr_api.hip; nothing is launched for 0 bytes).  Returns
// hipGetLastError() after the launch: a sticky error of an earlier launch of the same driver surfaces here, at the next
// zeroing, and not only at the driver's final check.
// Every driver zeroes through this and none through hipMemsetAsync: the memset node that a captured hipMemsetAsync
// becomes is not replayed reliably (tools/graph_memset_probe.py, profiles/graph_memset_probe.txt: six memsets of
// 12 .. 36 012 bytes in one graph are right on the first replay and hold 0x50 / 0xfe bytes and pointer-like words from
// the second on; the channel pullback's six already on the first).  What is left of hipMemsetAsync in the library:
//  * rocPRIM's onesweep radix sort (more than 2^20 keys) clears its histogram with it: dpr_sort.hip refuses such a
//    sort on a stream that is being captured;
//  * dpr_comm.hip's 0xff fill of a failed rank's gradients, in front of a collective that no graph holds.
hipError_t zero_async(hipStream_t st, void* p, size_t bytes);

bool tiled_supported(int n_out, const int64_t* grid);
bool tiled_preferred(int op, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t G);
size_t tiled_workspace_bytes(size_t elem, int op, unsigned flags, int n_in, int n_out,
                             const int64_t* grid, int64_t P, int64_t B);
bool tiled_batch_share_ok(int n_out, const int64_t* grid, int64_t P, int64_t B);
int tiled_tiles(int n_out, const int64_t* grid);
int tiled_slabs(int n_out, const int64_t* grid);  // 1: one piece; > 1: slabs along the last axis; 0: unsupported

template <typename T, int NI, int NO>
int raster_tiled(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out,
                 const T* points, const T* rot, const T* trans, const T* bg, const T* ow,
                 const T* pw, void* ws, size_t ws_bytes);

template <typename T, int NI, int NO>
int pullback_tiled(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P, int64_t B,
                   const T* g, const T* points, const T* rot, const T* trans, const T* ow,
                   const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw,
                   void* ws, size_t ws_bytes, Residual<T> rs);

// multi-channel forward on DPR_ALGO_TILED (per-pose binning of single-slab grids; dpr_tiled.hip)
bool tiled_channels_supported(int n_out, const int64_t* grid, int64_t P);
size_t tiled_channels_workspace_bytes(size_t elem, int n_in, int n_out, const int64_t* grid, int64_t P,
                                      int64_t B, int C);
template <typename T, int NI, int NO>
int raster_tiled_channels(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* out,
                          const T* points, const T* rot, const T* trans, const T* bg, const T* ow,
                          const T* pw, void* ws, size_t ws_bytes);

// forward-mode derivative on DPR_ALGO_TILED (the channel forward's per-pose binning; dpr_tiled.hip)
size_t tiled_jvp_workspace_bytes(size_t elem, int n_in, int n_out, const int64_t* grid, int64_t P);
template <typename T, int NI, int NO>
int raster_tiled_jvp(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out_dot,
                     const T* points, const T* rot, const T* trans, const T* ow, const T* pw, JvpTangents<T> tan,
                     const T* bg_dot, void* ws, size_t ws_bytes);

// DPR_ALGO_CHUNKED on 2-D grids: chunk-owned LDS tiles, pose loop inside (dpr_chunkown.hip)
size_t chunkown_workspace_bytes(size_t elem, int op, unsigned flags, int n_in, int64_t P,
                                int64_t B);
template <typename T, int NI>
int raster_chunkown(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P,
                    int64_t B, T* out, const T* points, const T* rot, const T* trans, const T* bg,
                    const T* ow, const T* pw, void* ws, size_t ws_bytes);
template <typename T, int NI>
int pullback_chunkown(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P,
                      int64_t B, const T* g, const T* points, const T* rot, const T* trans,
                      const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow,
                      T* d_pw, void* ws, size_t ws_bytes, Residual<T> rs);

// DPR_ALGO_CHUNKED on 3-D grids, sparse clouds over several poses: chunk lists (dpr_chunked.hip)
bool chunked_supported(int n_out, const int64_t* grid);
size_t chunked_workspace_bytes(int n_out, const int64_t* grid, int64_t P, int64_t B);
template <typename T, int NI, int NO>
int raster_chunked(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P,
                   int64_t B, T* out, const T* points, const T* rot, const T* trans, const T* bg,
                   const T* ow, const T* pw, void* ws, size_t ws_bytes);

// DPR_ALGO_CHUNKED on 3-D grids: owner-computes tiles over a box hierarchy, direct pullback (dpr_owner.hip)
size_t coarse_sort_scratch_bytes(size_t elem, int64_t P);
template <typename T>
int coarse_sort_with_perm(hipStream_t st, int n_in, int64_t P, const T* points, const T* pw, T* points_sorted,
                          T* pw_sorted, uint32_t* perm, char* scratch);
bool owner_supported(const int64_t* grid);
int64_t owner_tiles(const int64_t* grid);  // 32 x 32 x 14-cell tiles of the owner-computes forward
size_t owner_workspace_bytes(int op, const int64_t* grid, int64_t P, int64_t B);

template <typename T>
int raster_owner(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P, int64_t B,
                 T* out, const T* points, const T* rot, const T* trans, const T* bg, const T* ow,
                 const T* pw, void* ws, size_t ws_bytes);

template <typename T>
int pullback_owner(hipStream_t st, unsigned flags, const int64_t* grid, int64_t G, int64_t P, int64_t B,
                   const T* g, const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                   T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws, size_t ws_bytes);

// dpr_sort.hip: Hilbert sort of a cloud (keys, radix sort, gather); `fine`: 30-bit keys for 3-D clouds
size_t sort_workspace_bytes(int64_t P);
template <typename T>
int sort_points_impl(void* stream, int n_in, int64_t P, const T* points, T* points_sorted, uint32_t* perm,
                     const T* pw, T* pw_sorted, void* ws_, size_t ws_bytes, uint32_t* inv_perm, bool fine);

}  // namespace dpr
