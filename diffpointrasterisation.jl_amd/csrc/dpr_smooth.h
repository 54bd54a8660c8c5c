// The smooth splat (include/dpr.h, "SMOOTH SPLAT"): quadratic B-spline weights on 3^N cells per point.
// The launchers of dpr_smooth.hip, dpr_smooth_channels.hip, dpr_sample_smooth_channels.hip,
// dpr_sample_smooth_clouds.hip, dpr_smooth_bodies.hip and dpr_sample_smooth_bodies.hip that dpr_api_smooth.hip and dpr_api_smooth_bodies.hip call.  The tiles of
// DPR_ALGO_TILED (SmoothTileShape, SmoothTiles, smooth_tiles) and their index arithmetic, shared by the host plan and
// every key and tile kernel: dpr_smooth_tile.h.
#pragma once
#include <type_traits>

#include "../../include/dpr.h"
#include "dpr_smooth_tile.h"
#include "dpr_tiled.h"

namespace dpr {

constexpr uint32_t kSmoothNoKey = 0xffffffffu;  // a rejected point; sorts behind every tile

// (2,2), (3,3), (3,2): the pairs the smooth splat is compiled for
constexpr bool smooth_dims_supported(int n_in, int n_out) {
    return (n_in == 2 && n_out == 2) || (n_in == 3 && n_out == 3) || (n_in == 3 && n_out == 2);
}
// f(std::integral_constant<int, NI>{}, std::integral_constant<int, NO>{}) for the runtime pair.  Callers have refused
// every other pair with their family's own message.
template <class F> int with_smooth_dims(int n_in, int n_out, F&& f) {
    if (n_in == 2 && n_out == 2) return f(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
    if (n_in == 3 && n_out == 3) return f(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
    if (n_in == 3 && n_out == 2) return f(std::integral_constant<int, 3>{}, std::integral_constant<int, 2>{});
    return fail(DPR_ERR_UNSUPPORTED_DIMS, "smooth splat: unsupported (n_in, n_out) = (%d, %d)", n_in, n_out);
}

// tiles of the grid, or 0 where DPR_ALGO_TILED cannot run the call: tile ids 0 .. tiles - 1 must stay below the
// all-ones key and the index of a point must fit 32 bits (P <= 2^32 - 2)
int64_t smooth_tile_count(int n_out, const int64_t* grid, int64_t P);
// the message of every refusal that follows from smooth_tile_count == 0
constexpr char kSmoothTiledRefused[] = "smooth DPR_ALGO_TILED: too many tiles for a 32-bit key or P > 2^32 - 2";
// bytes of workspace of the tiled forward (0 for P = 0; (size_t)-1 where refused); independent of B:
// smooth_clouds_tiled_workspace_bytes (below) for a group of one
size_t smooth_tiled_workspace_bytes(int n_out, const int64_t* grid, int64_t P);

// The point kernels.  `out` holds the background already; the pullback's per-pose sums are zeroed and
// ds_dbackground is done by the caller (dpr_api_smooth.hip).
template <typename T, int NI, int NO>
int smooth_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                      const T* rot, const T* trans, const T* ow, const T* pw);
template <typename T, int NI, int NO>
int smooth_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                     const T* rot, const T* trans, const T* ow, const T* pw, void* ws, size_t ws_bytes);
// poses_per_slice / slices: the pose slicing of the linear atomic pullback (pose_slices of dpr_host.h); with
// more than one slice ds_dpoints / ds_dpoint_weight are zeroed here and added with atomics
template <typename T, int NI, int NO>
int smooth_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                      const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                      T* d_trans, T* d_ow, T* d_pw, int poses_per_slice, int64_t slices);

// The binning of DPR_ALGO_TILED, shared by every tiled launcher of dpr_smooth.hip, dpr_smooth_channels.hip and
// dpr_smooth_bodies.hip (the plan of the workspace, k_smooth_keys and k_smooth_ranges are compiled in dpr_smooth.hip
// only).  A call bins `group` images at a time: 1 for the families that bin pose by pose, smooth_clouds_group(...) for
// per-pose clouds and rigid bodies.
// smooth_binning: the tiles of a call and the pieces of its workspace, laid out for (group * tiles, group * P) and
//   reused from group to group -- the last may hold B % group images.  DPR_ERR_UNSUPPORTED_ALGO with
//   kSmoothTiledRefused where group is 0 or smooth_tile_count refuses, DPR_ERR_WORKSPACE where ws is too small.
// smooth_sort_group: what follows the key kernel of a family for nb images of P points: mark, stable radix sort of
//   the nb * P (key, index) pairs over the bits of nb * tiles, mark, start table (k_smooth_ranges: start[k] = first
//   sorted position with key >= k, k = 0 .. nb * tiles), mark.  Afterwards sb.start[k] .. sb.start[k + 1] is the run
//   of key k in sb.idx_out.
// smooth_bin_pose: k_smooth_keys of pose b, then smooth_sort_group of one image; depends on the primal only.
template <int NO> struct SmoothBinning {
    GridDesc<NO> gd;
    SmoothTiles<NO> tl;
    int64_t tiles;  // of one image
    int64_t group;  // images binned at a time
    char* temp;
    size_t temp_bytes;
    uint32_t *keys_in, *keys_out, *idx_in, *idx_out, *start;
};
template <int NO>
int smooth_binning(const int64_t* grid, int64_t G, int64_t P, int64_t B, int64_t group, void* ws, size_t ws_bytes,
                   SmoothBinning<NO>* sb);
template <int NO> int smooth_sort_group(hipStream_t st, const SmoothBinning<NO>& sb, int64_t nb, int64_t P);
template <typename T, int NI, int NO>
int smooth_bin_pose(hipStream_t st, const SmoothBinning<NO>& sb, int64_t P, int64_t b, const T* points, const T* rot,
                    const T* trans);

// C weights per point (include/dpr.h, "SMOOTH SPLAT, MULTI-CHANNEL"; kernels: dpr_smooth_channels.hip): pw is
// P x C with a point's weights contiguous, plane (c, b) of out / g at (b * C + c) * G.  The same contract with the
// caller as above: `out` holds the B * C backgrounds already, the per-pose sums are zeroed and ds_dbackground is done
// by the caller.  The tiled forward takes smooth_fwd_tiled's workspace and bins every pose once for all C channels.
// The pullback is one launch for all C channels; d_pw is P x C (NULL: not wanted).
template <typename T, int NI, int NO>
int smooth_channels_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* out,
                               const T* points, const T* rot, const T* trans, const T* ow, const T* pw);
template <typename T, int NI, int NO>
int smooth_channels_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* out,
                              const T* points, const T* rot, const T* trans, const T* ow, const T* pw, void* ws,
                              size_t ws_bytes);
template <typename T, int NI, int NO>
int smooth_channels_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, const T* g,
                               const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts,
                               T* d_rot, T* d_trans, T* d_ow, T* d_pw, int poses_per_slice, int64_t slices);

// Per-pose clouds (include/dpr.h, "SMOOTH SPLAT, PER-POSE CLOUDS"): cloud b at points + b * P * NI, its weights at
// pw + b * P, and ds_dpoints / ds_dpoint_weight likewise.  The same contract with the caller as above.
// The tiled forward bins a GROUP of poses with one key pass, one sort, one start table and one tile launch.
// Poses per group: the largest bg <= B with bg * max(P, tiles) <= kSmoothCloudsGroupWork, at least 1, at most
// max_group where that is > 0 (DPR_FLAG_MAX_POSE_GROUP); 0 where smooth_tile_count refuses the shape.  With bg > 1
// the keys b_local * tiles + tile stay below 2^24 and the flat indices b_local * P + p too.  (The value and the
// reason for it: include/dpr.h.)
constexpr int64_t kSmoothCloudsGroupWork = (int64_t)1 << 24;
int64_t smooth_clouds_group(int n_out, const int64_t* grid, int64_t P, int64_t B, int max_group);
// bytes of workspace of the tiled forward: the plan smooth_binning lays out for a group of smooth_clouds_group(...)
// images, reused from group to group; (size_t)-1 where refused
size_t smooth_clouds_tiled_workspace_bytes(int n_out, const int64_t* grid, int64_t P, int64_t B, int max_group);
template <typename T, int NI, int NO>
int smooth_clouds_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out,
                             const T* points, const T* rot, const T* trans, const T* ow, const T* pw);
template <typename T, int NI, int NO>
int smooth_clouds_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int max_group,
                            T* out, const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                            void* ws, size_t ws_bytes);
// one thread per (point, pose): no pose slices, every point gradient one plain store
template <typename T, int NI, int NO>
int smooth_clouds_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                             const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts,
                             T* d_rot, T* d_trans, T* d_ow, T* d_pw);

// Forward-mode derivative (include/dpr.h, "SMOOTH SPLAT, FORWARD MODE"): the deposits of K tangents added onto
// out_dot, whose planes (b * K + k) hold the background tangent already (jvp_fill of dpr_host.h, called by
// dpr_api_smooth.hip).  The tiled form takes smooth_fwd_tiled's workspace and bins every pose once for all K tangents.
template <typename T, int NI, int NO>
int smooth_jvp_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out_dot,
                      const T* points, const T* rot, const T* trans, const T* ow, const T* pw, JvpTangents<T> tan);
template <typename T, int NI, int NO>
int smooth_jvp_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out_dot,
                     const T* points, const T* rot, const T* trans, const T* ow, const T* pw, JvpTangents<T> tan,
                     void* ws, size_t ws_bytes);

// Rigid bodies (include/dpr.h, "SMOOTH SPLAT, RIGID BODIES" and "... FORWARD MODE"; kernels: dpr_smooth_bodies.hip):
// point p is seen in image b through pose b * K + body[p]; V tangents.  The same contract with the caller as above
// (dpr_api_smooth_bodies.hip).  The tiled forms bin the images in groups as smooth_clouds_fwd_tiled bins poses and
// take its workspace; the JVP's binning serves all V tangents.  The pullback slices the images as smooth_bwd_atomic
// slices the poses, and zeroes d_pts / d_pw here with more than one slice.
template <typename T, int NI, int NO>
int smooth_bodies_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out,
                             const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                             const T* pw);
template <typename T, int NI, int NO>
int smooth_bodies_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int max_group,
                            T* out, const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                            const T* pw, void* ws, size_t ws_bytes);
// the binning of the images b0 .. b0 + nb - 1 (k_smooth_bodies_keys, then smooth_sort_group): what the tiled launchers
// of dpr_smooth_bodies.hip and of dpr_sample_smooth_bodies.hip run before their tile kernels
template <typename T, int NI, int NO>
int smooth_bodies_bin_group(hipStream_t st, const SmoothBinning<NO>& sb, int64_t P, int64_t b0, int64_t nb, int K,
                            const T* points, const int32_t* body, const T* rot, const T* trans);
template <typename T, int NI, int NO>
int smooth_bodies_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, const T* g,
                             const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                             const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_ow, T* d_pw, int poses_per_slice,
                             int64_t slices);
template <typename T, int NI, int NO>
int smooth_bodies_jvp_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int V,
                             T* out_dot, const T* points, const int32_t* body, const T* rot, const T* trans,
                             const T* ow, const T* pw, JvpTangents<T> tan);
template <typename T, int NI, int NO>
int smooth_bodies_jvp_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int V,
                            int max_group, T* out_dot, const T* points, const int32_t* body, const T* rot,
                            const T* trans, const T* ow, const T* pw, JvpTangents<T> tan, void* ws, size_t ws_bytes);

// Smooth sampling (include/dpr.h, "SMOOTH SAMPLING"), with the same pose slicing.  Forward: values (P x B, point
// index fastest) are stored, no atomics.  Pullback: any of d_img, d_pts, d_rot, d_trans may be NULL (none: nothing
// is launched); d_img, d_rot and d_trans are zeroed by the caller, d_pts here when there is more than one slice;
// `image` is read only for d_pts / d_rot / d_trans.
template <typename T, int NI, int NO>
int sample_smooth_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* values, const T* image,
                      const T* points, const T* rot, const T* trans, int poses_per_slice, int64_t slices);
template <typename T, int NI, int NO>
int sample_smooth_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* dv,
                      const T* image, const T* points, const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot,
                      T* d_trans, int poses_per_slice, int64_t slices);

// Smooth sampling of C-channel images (include/dpr.h, "SMOOTH SAMPLING, MULTI-CHANNEL"; kernels:
// dpr_sample_smooth_channels.hip): image / d_img as `out` of the smooth channel splat (plane (c, b) at
// (b * C + c) * G), values / dv with a point's C values contiguous and the pose slowest ((b * P + p) * C + c), so that
// column b of dv is a `pw` of smooth_channels_fwd_tiled.  The same contract with the caller (dpr_api_smooth.hip) as
// sample_smooth_fwd / sample_smooth_bwd: d_img (B * C planes), d_rot and d_trans are zeroed by the caller.
template <typename T, int NI, int NO>
int sample_smooth_channels_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* values,
                               const T* image, const T* points, const T* rot, const T* trans, int poses_per_slice,
                               int64_t slices);
template <typename T, int NI, int NO>
int sample_smooth_channels_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C,
                               const T* dv, const T* image, const T* points, const T* rot, const T* trans, T* d_img,
                               T* d_pts, T* d_rot, T* d_trans, int poses_per_slice, int64_t slices);

// Smooth sampling at per-pose clouds (include/dpr.h, "SMOOTH SAMPLING, PER-POSE CLOUDS"; kernels:
// dpr_sample_smooth_clouds.hip): cloud b at points + b * P * NI and d_pts likewise, values / dv (B, P) with the point
// index fastest -- dv is a `pw` of smooth_clouds_fwd_tiled.  One thread per (point, pose), no pose slices: d_pts is
// stored, never zeroed or accumulated.  d_img, d_rot and d_trans are zeroed by the caller (dpr_api_smooth.hip); any of
// the four outputs may be NULL (none: nothing is launched); `image` is read only for d_pts / d_rot / d_trans.
template <typename T, int NI, int NO>
int sample_smooth_clouds_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* values,
                             const T* image, const T* points, const T* rot, const T* trans);
template <typename T, int NI, int NO>
int sample_smooth_clouds_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* dv,
                             const T* image, const T* points, const T* rot, const T* trans, T* d_img, T* d_pts,
                             T* d_rot, T* d_trans);

// Smooth sampling at the points of rigid bodies (include/dpr.h, "SMOOTH SAMPLING, RIGID BODIES"; kernels:
// dpr_sample_smooth_bodies.hip): smooth sampling through pose b * K + body[p].  The same contract with the caller
// (dpr_api_smooth_bodies.hip) as sample_smooth_fwd / sample_smooth_bwd; d_rot and d_trans hold B * K poses.
// sample_smooth_bodies_image_tiled adds ds_dimage onto zeroed planes: the images binned in groups as
// smooth_bodies_fwd_tiled bins them, with its workspace, the weight of (point, image) read from dv.
template <typename T, int NI, int NO>
int sample_smooth_bodies_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* values,
                             const T* image, const T* points, const int32_t* body, const T* rot, const T* trans,
                             int poses_per_slice, int64_t slices);
template <typename T, int NI, int NO>
int sample_smooth_bodies_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, const T* dv,
                             const T* image, const T* points, const int32_t* body, const T* rot, const T* trans,
                             T* d_img, T* d_pts, T* d_rot, T* d_trans, int poses_per_slice, int64_t slices);
template <typename T, int NI, int NO>
int sample_smooth_bodies_image_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K,
                                     int max_group, T* d_img, const T* dv, const T* points, const int32_t* body,
                                     const T* rot, const T* trans, void* ws, size_t ws_bytes);

}  // namespace dpr
