// The smooth entry points of libdpr -- splat, sampling, forward mode, per-pose clouds and sampling at them, weight
// channels and sampling of channel images: what each family is, its AUTO rule, its extent and size bounds, and the C
// ABI.  The checks, pointer checks, stream prologues and entry-point skeletons they share: dpr_host_smooth.h (core:
// dpr_api.hip; kernels and their launches: dpr_smooth.hip, dpr_smooth_channels.hip, dpr_sample_smooth_channels.hip,
// dpr_sample_smooth_clouds.hip; the smooth splat of rigid bodies: dpr_api_smooth_bodies.hip).
#include <hip/hip_runtime.h>

#include "dpr_host_smooth.h"

namespace dpr {

static int no_extent() { return DPR_OK; }

// ---------------------------------------------------------------- smooth splat
// dpr_raster_smooth_ex_* / dpr_raster_pullback_smooth_ex_* (include/dpr.h, "SMOOTH SPLAT"; kernels: dpr_smooth.hip).
// (2,2), (3,3), (3,2) only.  DPR_ALGO_ATOMIC: forward and pullback; DPR_ALGO_TILED: forward.
constexpr SmoothFamily kSmoothSplat{"smooth splat", kTiledForward, /*residual_refusal*/ true, /*group_plan*/ false,
                                    kGroupIgnored, /*has_body*/ false, /*needs_point_weight*/ false,
                                    /*pullback_slices_poses*/ true};

// AUTO (dpr_resolve_algo_smooth), from the shape alone (profiles/smooth_probe.txt, fp32, uniform clouds in either
// order, 1 and 16 poses).  The pullback is DPR_ALGO_ATOMIC.  The forward is DPR_ALGO_TILED from a point count on,
// where the tile ids fit the sort key, and DPR_ALGO_ATOMIC below it: the tiled path pays a sort and four launches
// per pose (0.07-0.1 ms), the atomic one 3^N atomics per point.
//  - 3-D grids, from 1e5 points: 1e5 -> 128^3 0.113 against 0.145 ms (16 poses 1.24 / 1.70), -> 256^3 0.149 / 0.148
//    (16 poses 1.98 / 1.84: the one row where the rule loses, 1.08x); 3e4 -> 128^3 0.091 against 0.071 ATOMIC;
//    1e7 -> 256^3 0.64 against 9.9 ms.
//  - 2-D grids, from 5e5 points (9 atomics per point, not 27): 3e5 -> 512^2 0.173 against 0.148 ms ATOMIC (16 poses
//    2.21 / 1.82), 1e6 0.229 against 0.412 (3.14 / 5.98).  Between 3e5 and 1e6 nothing was measured.
constexpr int64_t kSmoothTiledMinPoints3D = 100000;
constexpr int64_t kSmoothTiledMinPoints2D = 500000;
static int resolve_algo_smooth(int op, int n_out, const int64_t* grid, int64_t P) {
    const int64_t min_points = n_out == 3 ? kSmoothTiledMinPoints3D : kSmoothTiledMinPoints2D;
    if (op == DPR_OP_RASTER && P >= min_points && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

// (the entry points alone hold P to the block count of a launch: this family's query and resolver answer for any P)
static SmoothCall check_smooth_splat(bool entry_point, int op, int algo, unsigned flags, int n_in, int n_out,
                                     const int64_t* grid, int64_t P, int64_t B) {
    return smooth_checks(
        kSmoothSplat, op, algo, flags, n_in, n_out, grid, P, B, no_extent,
        [&](int64_t) { return entry_point ? check_point_blocks(P) : DPR_OK; },
        [&] { return resolve_algo_smooth(op, n_out, grid, P); });
}

template <typename T>
static int raster_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, T* out, const T* points, const T* rot, const T* trans,
                              const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    const SmoothCall c = check_smooth_splat(true, DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B);
    return smooth_splat_forward<T>(
        kSmoothSplat, c, stream, n_in, n_out, P, B, B, out, points, nullptr, rot, trans, bg, ow, pw, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_fwd_tiled<T, NI, NO>(st, grid, c.G, P, B, out, points, rot, trans, ow, pw, ws, ws_bytes)
                       : smooth_fwd_atomic<T, NI, NO>(st, grid, c.G, P, B, out, points, rot, trans, ow, pw);
        });
}

template <typename T>
static int pullback_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, const T* g, const T* points, const T* rot, const T* trans,
                                const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw,
                                void* ws, size_t) {
    const SmoothCall c = check_smooth_splat(true, DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B);
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    return smooth_splat_pullback<T>(
        kSmoothSplat, c, stream, flags, n_in, n_out, P, B, B, B, g, points, nullptr, rot, trans, ow, pw, d_pts, d_rot,
        d_trans, d_bg, d_ow, d_pw, ws, [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return smooth_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
                slices);
        });
}

// ---------------------------------------------------------------- smooth sampling
// dpr_sample_smooth_ex_* / dpr_sample_smooth_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING"; kernels:
// dpr_smooth.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the fused kernel with image atomics;
// DPR_ALGO_TILED, the same kernel without them, then ds_dimage pose by pose from the tiled smooth forward.
constexpr SmoothFamily kSmoothSampling{"smooth sampling", kTiledPullback, /*residual_refusal*/ false,
                                       /*group_plan*/ false, kGroupIgnored, /*has_body*/ false,
                                       /*needs_point_weight*/ false, /*pullback_slices_poses*/ false};

// AUTO: the forward is ATOMIC; the pullback is TILED where the smooth forward of one pose of the shape would be
// (the measured rows: profiles/sample_smooth_probe.txt)
static int resolve_algo_sample_smooth(int op, int n_out, const int64_t* grid, int64_t P) {
    if (op == DPR_OP_PULLBACK) return resolve_algo_smooth(DPR_OP_RASTER, n_out, grid, P);
    return DPR_ALGO_ATOMIC;
}

// (the entry points and the query hold the sizes to check_sample_sizes: this family's resolver answers for any)
static SmoothCall check_sample_smooth(bool resolver, int op, int algo, unsigned flags, int n_in, int n_out,
                                      const int64_t* grid, int64_t P, int64_t B) {
    return smooth_checks(
        kSmoothSampling, op, algo, flags, n_in, n_out, grid, P, B, no_extent,
        [&](int64_t G) { return resolver ? DPR_OK : check_sample_sizes(P, B, G); },
        [&] { return resolve_algo_sample_smooth(op, n_out, grid, P); });
}

template <typename T>
static int sample_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, T* values, const T* image, const T* points, const T* rot,
                              const T* trans, void* ws, size_t) {
    const SmoothCall c = check_sample_smooth(false, DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B);
    return smooth_sample_forward<T>(
        kSmoothSampling, c, stream, n_in, n_out, P, B, values, image, points, nullptr, rot, trans, ws,
        [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return sample_smooth_fwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, values, image, points, rot, trans, poses_per_slice, slices);
        });
}

template <typename T>
static int sample_smooth_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, const T* dv, const T* image,
                                       const T* points, const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot,
                                       T* d_trans, void* ws, size_t ws_bytes) {
    const SmoothCall c = check_sample_smooth(false, DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B);
    return smooth_sample_pullback<T>(
        kSmoothSampling, c, stream, n_in, n_out, P, B, B, B, dv, image, points, nullptr, rot, trans, d_img, d_pts,
        d_rot, d_trans, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no, T* d_img_atomic, int poses_per_slice, int64_t slices) {
            return sample_smooth_bwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, dv, image, points, rot, trans, d_img_atomic, d_pts, d_rot, d_trans,
                poses_per_slice, slices);
        },
        [&](hipStream_t st, auto ni, auto no) -> int {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            // plane b: the single-pose tiled smooth forward of weights ds_dvalues[:, b] (a contiguous column),
            // out_weight 1 -- what dpr_raster_smooth_ex_*(DPR_ALGO_TILED) returns for them
            for (int64_t b = 0; b < B; ++b)
                if (int rc = smooth_fwd_tiled<T, NI, NO>(st, grid, c.G, P, 1, d_img + b * c.G, points,
                                                         rot + b * (NO * NI), trans + b * NO, nullptr, dv + b * P, ws,
                                                         ws_bytes))
                    return rc;
            return DPR_OK;
        });
}

// ---------------------------------------------------------------- smooth splat, forward mode
// dpr_raster_smooth_jvp_ex_* (include/dpr.h, "SMOOTH SPLAT, FORWARD MODE"; kernels: dpr_smooth.hip).  k_jvp_fill
// writes the background tangent into every plane, then DPR_ALGO_ATOMIC (k_smooth_jvp_atomic) or DPR_ALGO_TILED
// (the tiled smooth forward's binning once per pose, k_smooth_tile_jvp over (tiles, K)) adds the deposits.
// AUTO (dpr_resolve_algo_smooth_jvp), from the shape and K alone (profiles/smooth_jvp_probe.txt, fp32, uniform clouds
// in generation order).  The tiled path pays the key, sort and start table once per pose, whatever K; the atomic one
// 3^N atomics per (point, tangent).  So the point count from which DPR_ALGO_TILED pays falls with K: the rule is the
// smooth forward's with P * K in the place of P, and for 2-D grids a lower constant.
//  - 3-D grids, P * K >= 1e5 (the forward's constant): 1e5 -> 256^3, K = 1 0.183 against 0.169 ms ATOMIC (1.08x, the
//    one row where the rule loses), K = 4 0.378 / 0.503, K = 12 0.98 / 1.43; 1e7 -> 256^3, K = 12 7.8 against 119 ms.
//  - 2-D grids, P * K >= 4e5.  The forward's 5e5 with P alone broke two rows: 1e5 x 16 poses -> 128^2 at K = 4, 1.59
//    against 2.57 ms ATOMIC (1.61x), and at K = 12, 1.65 against 7.29 (4.4x).  At K = 1 the same shape is 1.53
//    against 0.68 ATOMIC, and 1e6 -> 512^2 is 0.268 against 0.435: the constant lies between P * K = 1e5 and 4e5,
//    and 4e5 is the measured row.  Nothing was measured between.
constexpr int64_t kSmoothJvpTiledMinWork3D = 100000;
constexpr int64_t kSmoothJvpTiledMinWork2D = 400000;
static int resolve_algo_smooth_jvp(int n_out, const int64_t* grid, int64_t P, int64_t K) {
    const int64_t min_work = n_out == 3 ? kSmoothJvpTiledMinWork3D : kSmoothJvpTiledMinWork2D;
    if (P * K >= min_work && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

constexpr SmoothFamily kSmoothJvp{"smooth JVP", kTiledOnlyOp, /*residual_refusal*/ false, /*group_plan*/ false,
                                  kGroupIgnored, /*has_body*/ false, /*needs_point_weight*/ false,
                                  /*pullback_slices_poses*/ false};

static SmoothCall check_smooth_jvp(int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                                   int64_t B, int64_t K) {
    return smooth_checks(
        kSmoothJvp, DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, [&] { return check_jvp(K, 0u); },
        [&](int64_t G) {
            if (int rc = check_sample_sizes(P, B, G)) return rc;
            return check_plane_offsets(G, K, B);
        },
        [&] { return resolve_algo_smooth_jvp(n_out, grid, P, K); });
}

template <typename T>
static int raster_smooth_jvp_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                  int64_t P, int64_t B, int64_t K, T* out_dot, const T* points, const T* rot,
                                  const T* trans, const T* ow, const T* pw, JvpTangents<T> tan, const T* bg_dot,
                                  void* ws, size_t ws_bytes) {
    const SmoothCall c = check_smooth_jvp(algo, flags, n_in, n_out, grid, P, B, K);
    const int k = (int)K;
    return smooth_jvp_forward<T>(
        kSmoothJvp, c, stream, n_in, n_out, P, B, K, out_dot, points, nullptr, rot, trans, ow, pw, tan, bg_dot, ws,
        ws_bytes, [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_jvp_tiled<T, NI, NO>(st, grid, c.G, P, B, k, out_dot, points, rot, trans, ow, pw, tan,
                                                     ws, ws_bytes)
                       : smooth_jvp_atomic<T, NI, NO>(st, grid, c.G, P, B, k, out_dot, points, rot, trans, ow, pw,
                                                      tan);
        });
}

// ---------------------------------------------------------------- smooth splat, per-pose clouds
// dpr_raster_smooth_clouds_ex_* / dpr_raster_pullback_smooth_clouds_ex_* (include/dpr.h, "SMOOTH SPLAT, PER-POSE
// CLOUDS"; kernels: dpr_smooth.hip).  DPR_ALGO_ATOMIC: forward and pullback, one thread per (point, pose).
// DPR_ALGO_TILED: forward, the poses binned in groups (smooth_clouds_group; DPR_FLAG_MAX_POSE_GROUP honoured).
constexpr SmoothFamily kSmoothClouds{"smooth splat of per-pose clouds", kTiledForward, /*residual_refusal*/ true,
                                     /*group_plan*/ true, kGroupIgnored, /*has_body*/ false,
                                     /*needs_point_weight*/ false, /*pullback_slices_poses*/ false};

// AUTO (dpr_resolve_algo_smooth_clouds), from the shape alone (profiles/smooth_clouds_probe.txt, fp32, uniform clouds
// in generation order, times in ms TILED / ATOMIC).  The pullback is DPR_ALGO_ATOMIC.  The forward is DPR_ALGO_TILED
// where both hold, DPR_ALGO_ATOMIC otherwise:
//  - the default GROUP holds enough points, bg * P >= 1e5 on a 3-D grid and 4e5 on a 2-D grid: the key pass, the
//    sort, the start table and the tile launch are paid once per group of bg poses, so the smooth forward's rule is
//    applied to bg * P in the place of P.  3-D, 128^3: 1e4 x 4 poses 0.115 / 0.091, 3e4 x 4 0.141 / 0.174, 1e4 x 16
//    0.219 / 0.229, 1e5 x 16 0.357 / 1.71.  2-D, 128^2: 1e4 x 16 0.112 / 0.107, 1e4 x 32 0.171 / 0.169, 3e4 x 16
//    0.182 / 0.232 (512^2: 0.194 / 0.230), 1e4 x 64 0.198 / 0.287, 1e5 x 64 0.347 / 2.46.  The smooth forward's 5e5
//    would have lost the two 3e4 x 16 rows by 1.27x and 1.19x; between 3.2e5 and 4.8e5 nothing was measured.
//  - a cloud holds at least 4 points per tile of its pose's grid, P >= 4 * tiles: every non-empty (pose, tile)
//    workgroup zeroes and flushes its LDS tile whatever it holds.  256^3 (16 384 tiles): 1e4 x 16 poses 0.664 /
//    0.386 and 3e4 x 4 0.285 / 0.202 (0.6 and 1.8 points per tile), 1e5 x 4 0.388 / 0.489 and 1e5 x 16 1.13 / 1.84
//    (6.1); 128^3 (2048 tiles): 1e4 x 16 a tie at 4.9.  No 2-D row comes near this bound (512^2 has 256 tiles).
constexpr int64_t kSmoothCloudsTiledMinWork3D = 100000;
constexpr int64_t kSmoothCloudsTiledMinWork2D = 400000;
constexpr int64_t kSmoothCloudsTiledMinPointsPerTile = 4;
static int resolve_algo_smooth_clouds(int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothCloudsTiledMinWork3D : kSmoothCloudsTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    return bg * P >= min_work && P / kSmoothCloudsTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED : DPR_ALGO_ATOMIC;
}

// 64-bit offsets: cloud b starts at b * P * n_in, plane b at b * G
static int check_cloud_sizes(int n_in, int64_t P, int64_t B, int64_t G) {
    if (int rc = check_point_blocks(P)) return rc;
    if (B > 0 && (P > ((int64_t)1 << 60) / B / n_in || G > ((int64_t)1 << 62) / B))
        return fail(DPR_ERR_INVALID_ARG, "B * P * n_in or the image (G * B) too large");
    return DPR_OK;
}

static SmoothCall check_smooth_clouds(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                      int64_t P, int64_t B) {
    return smooth_checks(
        kSmoothClouds, op, algo, flags, n_in, n_out, grid, P, B, no_extent,
        [&](int64_t G) { return check_cloud_sizes(n_in, P, B, G); },
        [&] { return resolve_algo_smooth_clouds(op, n_out, grid, P, B); });
}

template <typename T>
static int raster_smooth_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, T* out, const T* points, const T* rot, const T* trans,
                                     const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    const SmoothCall c = check_smooth_clouds(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B);
    return smooth_splat_forward<T>(
        kSmoothClouds, c, stream, n_in, n_out, P, B, B, out, points, nullptr, rot, trans, bg, ow, pw, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_clouds_fwd_tiled<T, NI, NO>(st, grid, c.G, P, B, max_pose_group(flags), out, points,
                                                            rot, trans, ow, pw, ws, ws_bytes)
                       : smooth_clouds_fwd_atomic<T, NI, NO>(st, grid, c.G, P, B, out, points, rot, trans, ow, pw);
        });
}

template <typename T>
static int pullback_smooth_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, const T* g, const T* points,
                                       const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                                       T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws, size_t) {
    const SmoothCall c = check_smooth_clouds(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B);
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    return smooth_splat_pullback<T>(
        kSmoothClouds, c, stream, flags, n_in, n_out, P, B, B, B, g, points, nullptr, rot, trans, ow, pw, d_pts, d_rot,
        d_trans, d_bg, d_ow, d_pw, ws, [&](hipStream_t st, auto ni, auto no, int, int64_t) {
            return smooth_clouds_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw);
        });
}

// ---------------------------------------------------------------- smooth sampling at per-pose clouds
// dpr_sample_smooth_clouds_ex_* / dpr_sample_smooth_clouds_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING, PER-POSE
// CLOUDS"; kernels: dpr_sample_smooth_clouds.hip).  Forward: DPR_ALGO_ATOMIC, one thread per (point, pose).  Pullback:
// DPR_ALGO_ATOMIC, the fused kernel with image atomics; DPR_ALGO_TILED, the same kernel without them, then ds_dimage
// from the tiled forward of the smooth cloud splat, the poses binned in its groups (DPR_FLAG_MAX_POSE_GROUP honoured).
constexpr SmoothFamily kSmoothCloudSampling{"smooth sampling at per-pose clouds", kTiledPullback,
                                            /*residual_refusal*/ false, /*group_plan*/ true, kGroupIgnored,
                                            /*has_body*/ false, /*needs_point_weight*/ false,
                                            /*pullback_slices_poses*/ false, /*per_pose_clouds*/ true};

// AUTO: the forward is ATOMIC; the pullback is TILED where the forward of the smooth cloud splat of the shape would
// be.  That rule was measured for the splat; this op's own times: profiles/sample_smooth_clouds_probe.txt.
static int resolve_algo_sample_smooth_clouds(int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (op == DPR_OP_PULLBACK) return resolve_algo_smooth_clouds(DPR_OP_RASTER, n_out, grid, P, B);
    return DPR_ALGO_ATOMIC;
}

static SmoothCall check_sample_smooth_clouds(int op, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t* grid, int64_t P, int64_t B) {
    return smooth_checks(
        kSmoothCloudSampling, op, algo, flags, n_in, n_out, grid, P, B, no_extent,
        [&](int64_t G) {
            if (int rc = check_cloud_sizes(n_in, P, B, G)) return rc;
            // values[b, p] at b * P + p (smooth sampling's bound; the clouds' B * P * n_in is the tighter one today)
            if (B > 0 && P > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "P * B too large");
            return (int)DPR_OK;
        },
        [&] { return resolve_algo_sample_smooth_clouds(op, n_out, grid, P, B); });
}

template <typename T>
static int sample_smooth_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, T* values, const T* image, const T* points, const T* rot,
                                     const T* trans, void* ws, size_t) {
    const SmoothCall c = check_sample_smooth_clouds(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B);
    return smooth_sample_forward<T>(
        kSmoothCloudSampling, c, stream, n_in, n_out, P, B, values, image, points, nullptr, rot, trans, ws,
        [&](hipStream_t st, auto ni, auto no, int, int64_t) {
            return sample_smooth_clouds_fwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, values, image, points, rot, trans);
        });
}

template <typename T>
static int sample_smooth_clouds_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                              const int64_t* grid, int64_t P, int64_t B, const T* dv, const T* image,
                                              const T* points, const T* rot, const T* trans, T* d_img, T* d_pts,
                                              T* d_rot, T* d_trans, void* ws, size_t ws_bytes) {
    const SmoothCall c = check_sample_smooth_clouds(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B);
    return smooth_sample_pullback<T>(
        kSmoothCloudSampling, c, stream, n_in, n_out, P, B, B, B, dv, image, points, nullptr, rot, trans, d_img, d_pts,
        d_rot, d_trans, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no, T* d_img_atomic, int, int64_t) {
            return sample_smooth_clouds_bwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, dv, image, points, rot, trans, d_img_atomic, d_pts, d_rot, d_trans);
        },
        [&](hipStream_t st, auto ni, auto no) -> int {
            // ds_dvalues (B, P) is a point_weight of the smooth cloud splat: the planes are what
            // dpr_raster_smooth_clouds_ex_*(DPR_ALGO_TILED) adds for those weights with out_weight 1
            return smooth_clouds_fwd_tiled<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, max_pose_group(flags), d_img, points, rot, trans, nullptr, dv, ws, ws_bytes);
        });
}

// ---------------------------------------------------------------- smooth splat, C weights per point
// dpr_raster_smooth_channels_ex_* / dpr_raster_pullback_smooth_channels_ex_* (include/dpr.h, "SMOOTH SPLAT,
// MULTI-CHANNEL"; kernels: dpr_smooth_channels.hip).  fill_background / grid_sum serve the B * C planes as they are
// (plane k = b * C + c pairs with background[k]).  DPR_ALGO_ATOMIC: forward and pullback; DPR_ALGO_TILED: forward, the
// smooth forward's binning and workspace, once per pose for all C channels.
// AUTO (dpr_resolve_algo_smooth_channels), from the shape and C alone (profiles/smooth_channels_probe.txt, fp32,
// uniform clouds in random order, times in ms TILED / ATOMIC; tests/golden/smooth_channels_auto.json).  The pullback
// is DPR_ALGO_ATOMIC.  The tiled path pays the key pass, the sort and the start table once per pose, whatever C; the
// atomic one 3^N atomics per (point, channel).  So the rule is the smooth forward's with P * C in the place of P:
//  - 3-D grids, P * C >= 1e5 (the forward's constant; no row of this op lies below 3e5): 1e5 x 16 poses -> 128^3,
//    C = 3 1.75 / 5.05, C = 16 4.63 / 26.3; 1e6 -> 256^3, C = 4 0.663 / 4.03; 1e7 -> 256^3, C = 16 3.93 / 157.
//  - 2-D grids, P * C >= 3e5: 1e5 x 16 poses -> 128^2, C = 3 1.48 / 1.90 (1.29x; the 4e5 of the JVP rule would have
//    lost this row), C = 4 1.54 / 2.53, C = 16 1.63 / 9.32; 1e6 -> 512^2, C = 3 0.244 / 1.15.  With one weight that
//    shape is ATOMIC's (0.68 against 1.38 ms, profiles/smooth_jvp_probe.txt): the constant lies between P * C = 1e5
//    and 3e5, and 3e5 is the measured row.  Nothing was measured between.
constexpr int64_t kSmoothChannelsTiledMinWork3D = 100000;
constexpr int64_t kSmoothChannelsTiledMinWork2D = 300000;
static int resolve_algo_smooth_channels(int op, int n_out, const int64_t* grid, int64_t P, int64_t C) {
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothChannelsTiledMinWork3D : kSmoothChannelsTiledMinWork2D;
    if (P * C >= min_work && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

constexpr SmoothFamily kSmoothChannels{"smooth splat with channels", kTiledForward, /*residual_refusal*/ true,
                                       /*group_plan*/ false, kGroupIgnored, /*has_body*/ false,
                                       /*needs_point_weight*/ true, /*pullback_slices_poses*/ true};

static SmoothCall check_smooth_channels(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                        int64_t P, int64_t B, int64_t C) {
    return smooth_checks(
        kSmoothChannels, op, algo, flags, n_in, n_out, grid, P, B, [&] { return check_channel_count(C); },
        [&](int64_t G) {
            // 64-bit offsets: plane (c, b) starts at (b * C + c) * G, the weights of point p at p * C
            if (int rc = check_point_blocks(P)) return rc;
            return check_plane_offsets(G, C, B);
        },
        [&] { return resolve_algo_smooth_channels(op, n_out, grid, P, C); });
}

// fill_background / grid_sum serve the B * C planes as they are: ds_dbackground[b, c] = sum of plane b * C + c
template <typename T>
static int raster_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t C, T* out, const T* points,
                                       const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws,
                                       size_t ws_bytes) {
    const SmoothCall c = check_smooth_channels(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, C);
    const int ch = (int)C;
    return smooth_splat_forward<T>(
        kSmoothChannels, c, stream, n_in, n_out, P, B, B * C, out, points, nullptr, rot, trans, bg, ow, pw, ws,
        ws_bytes, [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_channels_fwd_tiled<T, NI, NO>(st, grid, c.G, P, B, ch, out, points, rot, trans, ow, pw,
                                                              ws, ws_bytes)
                       : smooth_channels_fwd_atomic<T, NI, NO>(st, grid, c.G, P, B, ch, out, points, rot, trans, ow,
                                                               pw);
        });
}

template <typename T>
static int pullback_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t* grid, int64_t P, int64_t B, int64_t C, const T* g,
                                         const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                                         T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws,
                                         size_t) {
    const SmoothCall c = check_smooth_channels(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B, C);
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    return smooth_splat_pullback<T>(
        kSmoothChannels, c, stream, flags, n_in, n_out, P, B, B * C, B, g, points, nullptr, rot, trans, ow, pw, d_pts,
        d_rot, d_trans, d_bg, d_ow, d_pw, ws,
        [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return smooth_channels_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)C, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw,
                poses_per_slice, slices);
        });
}

// ---------------------------------------------------------------- smooth sampling of C-channel images
// dpr_sample_smooth_channels_ex_* / dpr_sample_smooth_channels_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING,
// MULTI-CHANNEL"; kernels: dpr_sample_smooth_channels.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the
// fused kernel with C image atomics per cell; DPR_ALGO_TILED, the same kernel without them, then ds_dimage pose by
// pose from the tiled smooth channel forward -- one binning per pose for all C channels.
// AUTO: the forward is ATOMIC; the pullback is TILED where the smooth channel forward of one pose of the shape would
// be (resolve_algo_smooth_channels; the measured rows: profiles/sample_smooth_channels_probe.txt).
static int resolve_algo_sample_smooth_channels(int op, int n_out, const int64_t* grid, int64_t P,
                                               int64_t C) {
    if (op == DPR_OP_PULLBACK) return resolve_algo_smooth_channels(DPR_OP_RASTER, n_out, grid, P, C);
    return DPR_ALGO_ATOMIC;
}

constexpr SmoothFamily kSmoothChannelSampling{"smooth channel sampling", kTiledPullback, /*residual_refusal*/ false,
                                              /*group_plan*/ false, kGroupIgnored, /*has_body*/ false,
                                              /*needs_point_weight*/ false, /*pullback_slices_poses*/ false};

// (the workspace is the tiled smooth forward's for one pose, whatever B and C)
static SmoothCall check_sample_smooth_channels(int op, int algo, unsigned flags, int n_in, int n_out,
                                               const int64_t* grid, int64_t P, int64_t B, int64_t C) {
    return smooth_checks(
        kSmoothChannelSampling, op, algo, flags, n_in, n_out, grid, P, B, [&] { return check_channel_count(C); },
        [&](int64_t G) {
            if (int rc = check_sample_sizes(P, B, G)) return rc;
            // 64-bit offsets: plane (c, b) starts at (b * C + c) * G, the values of (point p, pose b) at
            // (b * P + p) * C
            if (B > 0 && (P > ((int64_t)1 << 62) / (B * C) || G > ((int64_t)1 << 62) / (B * C)))
                return fail(DPR_ERR_INVALID_ARG, "P * C * B or the image (G * C * B) too large");
            return (int)DPR_OK;
        },
        [&] { return resolve_algo_sample_smooth_channels(op, n_out, grid, P, C); });
}

template <typename T>
static int sample_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t C, T* values, const T* image,
                                       const T* points, const T* rot, const T* trans, void* ws, size_t) {
    const SmoothCall c = check_sample_smooth_channels(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, C);
    return smooth_sample_forward<T>(
        kSmoothChannelSampling, c, stream, n_in, n_out, P, B, values, image, points, nullptr, rot, trans, ws,
        [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return sample_smooth_channels_fwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)C, values, image, points, rot, trans, poses_per_slice, slices);
        });
}

template <typename T>
static int sample_smooth_channels_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t* grid, int64_t P, int64_t B, int64_t C, const T* dv,
                                                const T* image, const T* points, const T* rot, const T* trans,
                                                T* d_img, T* d_pts, T* d_rot, T* d_trans, void* ws, size_t ws_bytes) {
    const SmoothCall c = check_sample_smooth_channels(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B, C);
    const int ch = (int)C;
    return smooth_sample_pullback<T>(
        kSmoothChannelSampling, c, stream, n_in, n_out, P, B, B * C, B, dv, image, points, nullptr, rot, trans, d_img,
        d_pts, d_rot, d_trans, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no, T* d_img_atomic, int poses_per_slice, int64_t slices) {
            return sample_smooth_channels_bwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, ch, dv, image, points, rot, trans, d_img_atomic, d_pts, d_rot, d_trans,
                poses_per_slice, slices);
        },
        [&](hipStream_t st, auto ni, auto no) -> int {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            // the C planes of pose b: the single-pose tiled smooth channel forward of the weights
            // ds_dvalues[:, :, b] (P x C, contiguous), out_weight 1 -- what
            // dpr_raster_smooth_channels_ex_*(DPR_ALGO_TILED) returns for them
            for (int64_t b = 0; b < B; ++b)
                if (int rc = smooth_channels_fwd_tiled<T, NI, NO>(st, grid, c.G, P, 1, ch, d_img + b * C * c.G, points,
                                                                  rot + b * (NO * NI), trans + b * NO, nullptr,
                                                                  dv + b * P * C, ws, ws_bytes))
                    return rc;
            return DPR_OK;
        });
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_smooth(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    return dpr::resolver_value(dpr::check_smooth_splat(false, op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B));
}

#define DPR_DEFINE_SMOOTH(SUF, T)                                                                              \
    size_t dpr_workspace_bytes_smooth_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,          \
                                               const int64_t* grid, int64_t P, int64_t B) {                    \
        return dpr::query_value(dpr::check_smooth_splat(false, op, algo, flags, n_in, n_out, grid, P, B));     \
    }                                                                                                          \
    int dpr_raster_smooth_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,                \
                                   const int64_t* grid, int64_t P, int64_t B, T* out, const T* points,         \
                                   const T* rotation, const T* translation, const T* background,               \
                                   const T* out_weight, const T* point_weight, void* workspace,                \
                                   size_t workspace_bytes) {                                                   \
        return dpr::raster_smooth_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, out, points, rotation, \
                                          translation, background, out_weight, point_weight, workspace,        \
                                          workspace_bytes);                                                    \
    }                                                                                                          \
    int dpr_raster_pullback_smooth_ex_##SUF(                                                                   \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        const T* ds_dout, const T* points, const T* rotation, const T* translation, const T* out_weight,       \
        const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, T* ds_dbackground,          \
        T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {                     \
        return dpr::pullback_smooth_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, ds_dout, points,     \
                                            rotation, translation, out_weight, point_weight, ds_dpoints,       \
                                            ds_drotation, ds_dtranslation, ds_dbackground, ds_dout_weight,     \
                                            ds_dpoint_weight, workspace, workspace_bytes);                     \
    }
DPR_DEFINE_SMOOTH(f32, float)
DPR_DEFINE_SMOOTH(f64, double)
#undef DPR_DEFINE_SMOOTH

int dpr_resolve_algo_sample_smooth(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    return dpr::resolver_value(dpr::check_sample_smooth(true, op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B));
}

#define DPR_DEFINE_SAMPLE_SMOOTH(SUF, T)                                                                       \
    size_t dpr_workspace_bytes_sample_smooth_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,   \
                                                      const int64_t* grid, int64_t P, int64_t B) {             \
        return dpr::query_value(dpr::check_sample_smooth(false, op, algo, flags, n_in, n_out, grid, P, B));    \
    }                                                                                                          \
    int dpr_sample_smooth_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,                \
                                   const int64_t* grid, int64_t P, int64_t B, T* values, const T* image,       \
                                   const T* points, const T* rotation, const T* translation, void* workspace,  \
                                   size_t workspace_bytes) {                                                   \
        return dpr::sample_smooth_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, values, image, points, \
                                          rotation, translation, workspace, workspace_bytes);                  \
    }                                                                                                          \
    int dpr_sample_smooth_pullback_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,       \
                                            const int64_t* grid, int64_t P, int64_t B, const T* ds_dvalues,    \
                                            const T* image, const T* points, const T* rotation,                \
                                            const T* translation, T* ds_dimage, T* ds_dpoints,                 \
                                            T* ds_drotation, T* ds_dtranslation, void* workspace,              \
                                            size_t workspace_bytes) {                                          \
        return dpr::sample_smooth_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, ds_dvalues,   \
                                                   image, points, rotation, translation, ds_dimage,            \
                                                   ds_dpoints, ds_drotation, ds_dtranslation, workspace,       \
                                                   workspace_bytes);                                           \
    }
DPR_DEFINE_SAMPLE_SMOOTH(f32, float)
DPR_DEFINE_SAMPLE_SMOOTH(f64, double)
#undef DPR_DEFINE_SAMPLE_SMOOTH

int dpr_resolve_algo_smooth_jvp(int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t K) {
    return dpr::resolver_value(dpr::check_smooth_jvp(DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, K));
}

#define DPR_DEFINE_SMOOTH_JVP(SUF, T)                                                                          \
    size_t dpr_workspace_bytes_smooth_jvp_ex_##SUF(int algo, unsigned flags, int n_in, int n_out,              \
                                                   const int64_t* grid, int64_t P, int64_t B, int64_t K) {     \
        return dpr::query_value(dpr::check_smooth_jvp(algo, flags, n_in, n_out, grid, P, B, K));               \
    }                                                                                                          \
    int dpr_raster_smooth_jvp_ex_##SUF(                                                                        \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        int64_t K, T* out_dot, const T* points, const T* rotation, const T* translation, const T* out_weight,  \
        const T* point_weight, const T* points_dot, const T* rotation_dot, const T* translation_dot,           \
        const T* background_dot, const T* out_weight_dot, const T* point_weight_dot, void* workspace,          \
        size_t workspace_bytes) {                                                                              \
        return dpr::raster_smooth_jvp_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, out_dot, points, \
                                              rotation, translation, out_weight, point_weight,                 \
                                              dpr::JvpTangents<T>{points_dot, rotation_dot, translation_dot,   \
                                                                  out_weight_dot, point_weight_dot},           \
                                              background_dot, workspace, workspace_bytes);                     \
    }
DPR_DEFINE_SMOOTH_JVP(f32, float)
DPR_DEFINE_SMOOTH_JVP(f64, double)
#undef DPR_DEFINE_SMOOTH_JVP

int dpr_resolve_algo_smooth_clouds(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    return dpr::resolver_value(dpr::check_smooth_clouds(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B));
}

#define DPR_DEFINE_SMOOTH_CLOUDS(SUF, T)                                                                       \
    size_t dpr_workspace_bytes_smooth_clouds_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,   \
                                                      const int64_t* grid, int64_t P, int64_t B) {             \
        return dpr::query_value(dpr::check_smooth_clouds(op, algo, flags, n_in, n_out, grid, P, B));           \
    }                                                                                                          \
    int dpr_raster_smooth_clouds_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,         \
                                          const int64_t* grid, int64_t P, int64_t B, T* out, const T* points,  \
                                          const T* rotation, const T* translation, const T* background,        \
                                          const T* out_weight, const T* point_weight, void* workspace,         \
                                          size_t workspace_bytes) {                                            \
        return dpr::raster_smooth_clouds_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, out, points,    \
                                                 rotation, translation, background, out_weight, point_weight,  \
                                                 workspace, workspace_bytes);                                  \
    }                                                                                                          \
    int dpr_raster_pullback_smooth_clouds_ex_##SUF(                                                            \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        const T* ds_dout, const T* points, const T* rotation, const T* translation, const T* out_weight,       \
        const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, T* ds_dbackground,          \
        T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {                     \
        return dpr::pullback_smooth_clouds_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, ds_dout,      \
                                                   points, rotation, translation, out_weight, point_weight,    \
                                                   ds_dpoints, ds_drotation, ds_dtranslation, ds_dbackground,  \
                                                   ds_dout_weight, ds_dpoint_weight, workspace,                \
                                                   workspace_bytes);                                           \
    }
DPR_DEFINE_SMOOTH_CLOUDS(f32, float)
DPR_DEFINE_SMOOTH_CLOUDS(f64, double)
#undef DPR_DEFINE_SMOOTH_CLOUDS

int dpr_resolve_algo_sample_smooth_clouds(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    return dpr::resolver_value(dpr::check_sample_smooth_clouds(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B));
}

#define DPR_DEFINE_SAMPLE_SMOOTH_CLOUDS(SUF, T)                                                                \
    size_t dpr_workspace_bytes_sample_smooth_clouds_ex_##SUF(int op, int algo, unsigned flags, int n_in,       \
                                                             int n_out, const int64_t* grid, int64_t P,        \
                                                             int64_t B) {                                      \
        return dpr::query_value(dpr::check_sample_smooth_clouds(op, algo, flags, n_in, n_out, grid, P, B));    \
    }                                                                                                          \
    int dpr_sample_smooth_clouds_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,         \
                                          const int64_t* grid, int64_t P, int64_t B, T* values,                \
                                          const T* image, const T* points, const T* rotation,                  \
                                          const T* translation, void* workspace, size_t workspace_bytes) {     \
        return dpr::sample_smooth_clouds_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, values, image,  \
                                                 points, rotation, translation, workspace, workspace_bytes);   \
    }                                                                                                          \
    int dpr_sample_smooth_clouds_pullback_ex_##SUF(                                                            \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        const T* ds_dvalues, const T* image, const T* points, const T* rotation, const T* translation,         \
        T* ds_dimage, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, void* workspace,                     \
        size_t workspace_bytes) {                                                                              \
        return dpr::sample_smooth_clouds_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B,        \
                                                          ds_dvalues, image, points, rotation, translation,    \
                                                          ds_dimage, ds_dpoints, ds_drotation,                 \
                                                          ds_dtranslation, workspace, workspace_bytes);        \
    }
DPR_DEFINE_SAMPLE_SMOOTH_CLOUDS(f32, float)
DPR_DEFINE_SAMPLE_SMOOTH_CLOUDS(f64, double)
#undef DPR_DEFINE_SAMPLE_SMOOTH_CLOUDS

int dpr_resolve_algo_smooth_channels(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                     int64_t C) {
    return dpr::resolver_value(dpr::check_smooth_channels(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, C));
}

#define DPR_DEFINE_SMOOTH_CHANNELS(SUF, T)                                                                     \
    size_t dpr_workspace_bytes_smooth_channels_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out, \
                                                        const int64_t* grid, int64_t P, int64_t B, int64_t C) { \
        return dpr::query_value(dpr::check_smooth_channels(op, algo, flags, n_in, n_out, grid, P, B, C));      \
    }                                                                                                          \
    int dpr_raster_smooth_channels_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,       \
                                            const int64_t* grid, int64_t P, int64_t B, int64_t C, T* out,      \
                                            const T* points, const T* rotation, const T* translation,          \
                                            const T* background, const T* out_weight, const T* point_weight,   \
                                            void* workspace, size_t workspace_bytes) {                         \
        return dpr::raster_smooth_channels_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C, out,       \
                                                   points, rotation, translation, background, out_weight,      \
                                                   point_weight, workspace, workspace_bytes);                  \
    }                                                                                                          \
    int dpr_raster_pullback_smooth_channels_ex_##SUF(                                                          \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        int64_t C, const T* ds_dout, const T* points, const T* rotation, const T* translation,                 \
        const T* out_weight, const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation,        \
        T* ds_dbackground, T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {  \
        return dpr::pullback_smooth_channels_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C, ds_dout, \
                                                     points, rotation, translation, out_weight, point_weight,  \
                                                     ds_dpoints, ds_drotation, ds_dtranslation,                \
                                                     ds_dbackground, ds_dout_weight, ds_dpoint_weight,         \
                                                     workspace, workspace_bytes);                              \
    }
DPR_DEFINE_SMOOTH_CHANNELS(f32, float)
DPR_DEFINE_SMOOTH_CHANNELS(f64, double)
#undef DPR_DEFINE_SMOOTH_CHANNELS

int dpr_resolve_algo_sample_smooth_channels(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                            int64_t C) {
    return dpr::resolver_value(
        dpr::check_sample_smooth_channels(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, C));
}

#define DPR_DEFINE_SAMPLE_SMOOTH_CHANNELS(SUF, T)                                                              \
    size_t dpr_workspace_bytes_sample_smooth_channels_ex_##SUF(int op, int algo, unsigned flags, int n_in,     \
                                                               int n_out, const int64_t* grid, int64_t P,      \
                                                               int64_t B, int64_t C) {                         \
        return dpr::query_value(                                                                               \
            dpr::check_sample_smooth_channels(op, algo, flags, n_in, n_out, grid, P, B, C));                   \
    }                                                                                                          \
    int dpr_sample_smooth_channels_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,       \
                                            const int64_t* grid, int64_t P, int64_t B, int64_t C, T* values,   \
                                            const T* image, const T* points, const T* rotation,                \
                                            const T* translation, void* workspace, size_t workspace_bytes) {   \
        return dpr::sample_smooth_channels_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C, values,    \
                                                   image, points, rotation, translation, workspace,            \
                                                   workspace_bytes);                                           \
    }                                                                                                          \
    int dpr_sample_smooth_channels_pullback_ex_##SUF(                                                          \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        int64_t C, const T* ds_dvalues, const T* image, const T* points, const T* rotation,                    \
        const T* translation, T* ds_dimage, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation,                \
        void* workspace, size_t workspace_bytes) {                                                             \
        return dpr::sample_smooth_channels_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C,   \
                                                            ds_dvalues, image, points, rotation, translation,  \
                                                            ds_dimage, ds_dpoints, ds_drotation,               \
                                                            ds_dtranslation, workspace, workspace_bytes);      \
    }
DPR_DEFINE_SAMPLE_SMOOTH_CHANNELS(f32, float)
DPR_DEFINE_SAMPLE_SMOOTH_CHANNELS(f64, double)
#undef DPR_DEFINE_SAMPLE_SMOOTH_CHANNELS

}  // extern "C"
