// The smooth entry points of libdpr -- splat, sampling, forward mode, per-pose clouds, weight channels and sampling of
// channel images: host checks, AUTO rules and C ABI (core: dpr_api.hip; kernels and their launches: dpr_smooth.hip,
// dpr_smooth_channels.hip, dpr_sample_smooth_channels.hip; the smooth splat of rigid bodies: dpr_api_smooth_bodies.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_smooth.h"

namespace dpr {

// ---------------------------------------------------------------- smooth splat
// dpr_raster_smooth_ex_* / dpr_raster_pullback_smooth_ex_* (include/dpr.h, "SMOOTH SPLAT"; kernels: dpr_smooth.hip).
// (2,2), (3,3), (3,2) only.  DPR_ALGO_ATOMIC: forward and pullback; DPR_ALGO_TILED: forward.
// (before check_common: the grid of a pair without kernels is not looked at)
static int check_smooth_dims(int n_in, int n_out) {
    if (!smooth_dims_supported(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_DIMS,
                    "unsupported (n_in, n_out) = (%d, %d); the smooth splat supports (2,2), (3,3), (3,2)", n_in, n_out);
    return DPR_OK;
}
static int check_smooth(int op, unsigned flags) {
    if (op == DPR_OP_RESIDUAL_PULLBACK)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth splat has no residual pullback");
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "smooth splat: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the smooth splat keeps / reuses no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    return DPR_OK;
}

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
static int resolve_algo_smooth(int algo, int op, int n_out, const int64_t* grid, int64_t P) {
    if (algo != DPR_ALGO_AUTO) return algo;
    const int64_t min_points = n_out == 3 ? kSmoothTiledMinPoints3D : kSmoothTiledMinPoints2D;
    if (op == DPR_OP_RASTER && P >= min_points && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

// bytes of workspace, or (size_t)-1 (message recorded) when the algorithm cannot run the call
static size_t smooth_workspace_bytes(int op, int algo, int n_out, const int64_t* grid, int64_t P) {
    if (algo == DPR_ALGO_ATOMIC) return 0;  // (the pullback's per-pose partials leave their block as atomics)
    if (algo != DPR_ALGO_TILED) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth splat runs on DPR_ALGO_ATOMIC and DPR_ALGO_TILED, not algorithm %d",
             algo);
        return (size_t)-1;
    }
    if (op != DPR_OP_RASTER) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth pullback runs on DPR_ALGO_ATOMIC only");
        return (size_t)-1;
    }
    const size_t n = smooth_tiled_workspace_bytes(n_out, grid, P);
    if (n == (size_t)-1)
        fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    return n;
}

template <typename T>
static int raster_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, T* out, const T* points, const T* rot, const T* trans,
                              const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_smooth(DPR_OP_RASTER, flags)) return rc;
    if (int rc = check_point_blocks(P)) return rc;
    algo = resolve_algo_smooth(algo, DPR_OP_RASTER, n_out, grid, P);
    const size_t need = smooth_workspace_bytes(DPR_OP_RASTER, algo, n_out, grid, P);
    if (need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth splat (algorithm %d) needs %zu workspace bytes, got %zu", algo, need,
                    ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    fill_background(st, out, G, B, bg);
    stage_mark(st);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_fwd_tiled<T, NI, NO>(st, grid, G, P, B, out, points, rot, trans, ow, pw, ws, ws_bytes)
                           : smooth_fwd_atomic<T, NI, NO>(st, grid, G, P, B, out, points, rot, trans, ow, pw);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int pullback_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, const T* g, const T* points, const T* rot, const T* trans,
                                const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw,
                                void* ws, size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_smooth(DPR_OP_PULLBACK, flags)) return rc;
    if (int rc = check_point_blocks(P)) return rc;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    algo = resolve_algo_smooth(algo, DPR_OP_PULLBACK, n_out, grid, P);
    if (smooth_workspace_bytes(DPR_OP_PULLBACK, algo, n_out, grid, P) == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    if (B == 0) return DPR_OK;  // (every output is empty)
    if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (!d_rot || !d_trans || !d_bg || !d_ow) return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * n_out * n_in)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * n_out)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)B));
    grid_sum(st, g, G, B, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    if (P == 0) return DPR_OK;  // (the per-pose sums are 0, ds_dbackground is done; pose_slices divides by the blocks)
    int64_t slices = 1;
    const int poses_per_slice = pose_slices(P, B, &slices);  // (the linear atomic pullback's: SUMMATION ORDER, note 1)
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = smooth_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
            slices);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static size_t workspace_smooth_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                    int64_t P, int64_t B) {
    int64_t G = 0;
    if (check_smooth_dims(n_in, n_out)) return (size_t)-1;
    if (check_common(n_in, n_out, grid, P, B, &G)) return (size_t)-1;
    if (check_smooth(op, flags)) return (size_t)-1;
    algo = resolve_algo_smooth(algo, op, n_out, grid, P);
    return smooth_workspace_bytes(op, algo, n_out, grid, P);
}

// ---------------------------------------------------------------- smooth sampling
// dpr_sample_smooth_ex_* / dpr_sample_smooth_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING"; kernels:
// dpr_smooth.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the fused kernel with image atomics;
// DPR_ALGO_TILED, the same kernel without them, then ds_dimage pose by pose from the tiled smooth forward.
static int check_sample_smooth_op(int op, unsigned flags) {
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "smooth sampling: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth sampling keeps / reuses no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    return DPR_OK;
}

// AUTO: the forward is ATOMIC; the pullback is TILED where the smooth forward of one pose of the shape would be
// (the measured rows: profiles/sample_smooth_probe.txt)
static int resolve_algo_sample_smooth(int algo, int op, int n_out, const int64_t* grid, int64_t P) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op == DPR_OP_PULLBACK) return resolve_algo_smooth(DPR_ALGO_AUTO, DPR_OP_RASTER, n_out, grid, P);
    return DPR_ALGO_ATOMIC;
}

// bytes of workspace, or (size_t)-1 (message recorded) when the algorithm cannot run the call
static size_t sample_smooth_workspace_bytes(int op, int algo, int n_out, const int64_t* grid, int64_t P) {
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (algo != DPR_ALGO_TILED) {
        fail(DPR_ERR_UNSUPPORTED_ALGO,
             "smooth sampling runs on DPR_ALGO_ATOMIC and, the pullback, DPR_ALGO_TILED, not algorithm %d", algo);
        return (size_t)-1;
    }
    if (op != DPR_OP_PULLBACK) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth sampling forward runs on DPR_ALGO_ATOMIC only");
        return (size_t)-1;
    }
    const size_t n = smooth_tiled_workspace_bytes(n_out, grid, P);
    if (n == (size_t)-1)
        fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    return n;
}

// the host checks both entry points share; *G_out and the resolved *algo come back
static int check_sample_smooth(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                               int64_t B, int64_t* G_out, size_t* need) {
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, G_out)) return rc;
    if (int rc = check_sample_smooth_op(op, flags)) return rc;
    *algo = resolve_algo_sample_smooth(*algo, op, n_out, grid, P);
    *need = sample_smooth_workspace_bytes(op, *algo, n_out, grid, P);
    if (*need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    return check_sample_sizes(P, B, *G_out);
}

template <typename T>
static int sample_smooth_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, T* values, const T* image, const T* points, const T* rot,
                              const T* trans, void* ws, size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return rc;
    if (P == 0 || B == 0) return DPR_OK;
    if (!values) return fail(DPR_ERR_INVALID_ARG, "values is NULL");
    if (!image) return fail(DPR_ERR_INVALID_ARG, "image is NULL");
    if (!points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (int rc = check_alignment<T>(ws, {values, image, points, rot, trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = sample_smooth_fwd<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, values, image, points, rot, trans, pps, slices);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int sample_smooth_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, const T* dv, const T* image,
                                       const T* points, const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot,
                                       T* d_trans, void* ws, size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return rc;
    if (!d_img && !d_pts && !d_rot && !d_trans)
        return fail(DPR_ERR_INVALID_ARG, "smooth sampling pullback: every output is NULL");
    const bool tiled = algo == DPR_ALGO_TILED;
    if (tiled && d_img && P > 0 && B > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "DPR_ALGO_TILED smooth sampling pullback needs %zu workspace bytes, got %zu",
                    need, ws ? ws_bytes : (size_t)0);
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && B > 0) {
        if (!dv) return fail(DPR_ERR_INVALID_ARG, "ds_dvalues is NULL");
        if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
        if ((d_pts || d_rot || d_trans) && !image)
            return fail(DPR_ERR_INVALID_ARG, "image is NULL (needed for ds_dpoints / ds_drotation / ds_dtranslation)");
    }
    if (int rc = check_alignment<T>(ws, {dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    if (d_rot) DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * n_out * n_in)));
    if (d_trans) DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * n_out)));
    if (d_img) DPR_HIP(zero_async(st, d_img, sizeof(T) * (size_t)(B * G)));
    if (d_pts && B == 0) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
    if (P == 0 || B == 0) return DPR_OK;
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        if (int rc = sample_smooth_bwd<T, NI, NO>(st, grid, G, P, B, dv, image, points, rot, trans,
                                                  tiled ? nullptr : d_img, d_pts, d_rot, d_trans, pps, slices))
            return rc;
        stage_mark(st);
        if (tiled && d_img) {
            // plane b (zeroed above): the single-pose tiled smooth forward of weights ds_dvalues[:, b] (a contiguous
            // column), out_weight 1 -- what dpr_raster_smooth_ex_*(DPR_ALGO_TILED) returns for them
            for (int64_t b = 0; b < B; ++b)
                if (int rc = smooth_fwd_tiled<T, NI, NO>(st, grid, G, P, 1, d_img + b * G, points, rot + b * (NO * NI),
                                                         trans + b * NO, nullptr, dv + b * P, ws, ws_bytes))
                    return rc;
        }
        return DPR_OK;
    });
}

template <typename T>
static size_t workspace_sample_smooth_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                           int64_t P, int64_t B) {
    int64_t G = 0;
    size_t need = 0;
    if (check_sample_smooth(op, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return (size_t)-1;
    return need;
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
static int resolve_algo_smooth_jvp(int algo, int n_out, const int64_t* grid, int64_t P, int64_t K) {
    if (algo != DPR_ALGO_AUTO) return algo;
    const int64_t min_work = n_out == 3 ? kSmoothJvpTiledMinWork3D : kSmoothJvpTiledMinWork2D;
    if (P * K >= min_work && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

// the checks every smooth JVP entry point and query shares, in the smooth entry points' order; *need: workspace
static int check_smooth_jvp(int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                            int64_t B, int64_t K, int64_t* G, size_t* need) {
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (int rc = check_jvp(K, flags)) return rc;
    if (int rc = check_sample_sizes(P, B, *G)) return rc;
    if (B > 0 && *G * K > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "output too large");
    *algo = resolve_algo_smooth_jvp(*algo, n_out, grid, P, K);
    *need = smooth_workspace_bytes(DPR_OP_RASTER, *algo, n_out, grid, P);
    return *need == (size_t)-1 ? DPR_ERR_UNSUPPORTED_ALGO : DPR_OK;
}

template <typename T>
static int raster_smooth_jvp_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                  int64_t P, int64_t B, int64_t K, T* out_dot, const T* points, const T* rot,
                                  const T* trans, const T* ow, const T* pw, JvpTangents<T> tan, const T* bg_dot,
                                  void* ws, size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_jvp(&algo, flags, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
    if (B == 0) return DPR_OK;
    if (!out_dot) return fail(DPR_ERR_INVALID_ARG, "out_dot is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth JVP (algorithm %d) needs %zu workspace bytes, got %zu", algo, need,
                    ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out_dot, points, rot, trans, ow, pw, tan.points, tan.rot, tan.trans, tan.ow,
                                         tan.pw, bg_dot}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    // the background tangent (or 0) into every plane; then the deposits, where any other tangent is given
    const int k = (int)K;
    jvp_fill(st, out_dot, G, k, B, bg_dot);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    if (P == 0 || !(tan.points || tan.rot || tan.trans || tan.ow || tan.pw)) return DPR_OK;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_jvp_tiled<T, NI, NO>(st, grid, G, P, B, k, out_dot, points, rot, trans, ow, pw, tan,
                                                         ws, ws_bytes)
                           : smooth_jvp_atomic<T, NI, NO>(st, grid, G, P, B, k, out_dot, points, rot, trans, ow, pw,
                                                          tan);
        stage_mark(st);
        return rc;
    });
}

static size_t workspace_smooth_jvp_impl(int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                                        int64_t B, int64_t K) {
    int64_t G = 0;
    size_t need = 0;
    if (check_smooth_jvp(&algo, flags, n_in, n_out, grid, P, B, K, &G, &need)) return (size_t)-1;
    return need;
}

// ---------------------------------------------------------------- smooth splat, per-pose clouds
// dpr_raster_smooth_clouds_ex_* / dpr_raster_pullback_smooth_clouds_ex_* (include/dpr.h, "SMOOTH SPLAT, PER-POSE
// CLOUDS"; kernels: dpr_smooth.hip).  DPR_ALGO_ATOMIC: forward and pullback, one thread per (point, pose).
// DPR_ALGO_TILED: forward, the poses binned in groups (smooth_clouds_group; DPR_FLAG_MAX_POSE_GROUP honoured).

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
static int resolve_algo_smooth_clouds(int algo, int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothCloudsTiledMinWork3D : kSmoothCloudsTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    return bg * P >= min_work && P / kSmoothCloudsTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED : DPR_ALGO_ATOMIC;
}

// bytes of workspace, or (size_t)-1 (message recorded) when the algorithm cannot run the call
static size_t smooth_clouds_workspace_bytes(int op, int algo, unsigned flags, int n_out, const int64_t* grid,
                                            int64_t P, int64_t B) {
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (algo != DPR_ALGO_TILED) {
        fail(DPR_ERR_UNSUPPORTED_ALGO,
             "the smooth splat of per-pose clouds runs on DPR_ALGO_ATOMIC and DPR_ALGO_TILED, not algorithm %d", algo);
        return (size_t)-1;
    }
    if (op != DPR_OP_RASTER) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth pullback runs on DPR_ALGO_ATOMIC only");
        return (size_t)-1;
    }
    const size_t n = smooth_clouds_tiled_workspace_bytes(n_out, grid, P, B, max_pose_group(flags));
    if (n == (size_t)-1)
        fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    return n;
}

// the checks every entry point and query of the family shares, in the order of the two parent families; *G and the
// resolved *algo come back, *need: workspace
static int check_smooth_clouds(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                               int64_t B, int64_t* G, size_t* need) {
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (int rc = check_smooth(op, flags)) return rc;
    // 64-bit offsets: cloud b starts at b * P * n_in, plane b at b * G
    if (int rc = check_point_blocks(P)) return rc;
    if (B > 0 && (P > ((int64_t)1 << 60) / B / n_in || *G > ((int64_t)1 << 62) / B))
        return fail(DPR_ERR_INVALID_ARG, "B * P * n_in or the image (G * B) too large");
    *algo = resolve_algo_smooth_clouds(*algo, op, n_out, grid, P, B);
    *need = smooth_clouds_workspace_bytes(op, *algo, flags, n_out, grid, P, B);
    return *need == (size_t)-1 ? DPR_ERR_UNSUPPORTED_ALGO : DPR_OK;
}

template <typename T>
static int raster_smooth_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, T* out, const T* points, const T* rot, const T* trans,
                                     const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_clouds(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return rc;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth splat of per-pose clouds (algorithm %d) needs %zu workspace bytes, got %zu",
                    algo, need, ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    fill_background(st, out, G, B, bg);
    stage_mark(st);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_clouds_fwd_tiled<T, NI, NO>(st, grid, G, P, B, max_pose_group(flags), out,
                                                                points, rot, trans, ow, pw, ws, ws_bytes)
                           : smooth_clouds_fwd_atomic<T, NI, NO>(st, grid, G, P, B, out, points, rot, trans, ow, pw);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int pullback_smooth_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, const T* g, const T* points,
                                       const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                                       T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws, size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_clouds(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return rc;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    if (B == 0) return DPR_OK;  // (every output is empty)
    if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (!d_rot || !d_trans || !d_bg || !d_ow) return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * n_out * n_in)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * n_out)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)B));
    grid_sum(st, g, G, B, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = smooth_clouds_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw);
        stage_mark(st);
        return rc;
    });
}

static size_t workspace_smooth_clouds_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                           int64_t P, int64_t B) {
    int64_t G = 0;
    size_t need = 0;
    if (check_smooth_clouds(op, &algo, flags, n_in, n_out, grid, P, B, &G, &need)) return (size_t)-1;
    return need;
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
static int resolve_algo_smooth_channels(int algo, int op, int n_out, const int64_t* grid, int64_t P, int64_t C) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothChannelsTiledMinWork3D : kSmoothChannelsTiledMinWork2D;
    if (P * C >= min_work && smooth_tile_count(n_out, grid, P) != 0) return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

// the checks every entry point and query of the family shares, in the smooth entry points' order; *G and the
// resolved *algo come back, *need: workspace
static int check_smooth_channels(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                 int64_t P, int64_t B, int64_t C, int64_t* G, size_t* need) {
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (int rc = check_smooth(op, flags)) return rc;
    if (C < 1 || C > kMaxChannels)
        return fail(DPR_ERR_INVALID_ARG, "channels C = %lld out of range [1, %d]", (long long)C, kMaxChannels);
    // 64-bit offsets: plane (c, b) starts at (b * C + c) * G, the weights of point p at p * C
    if (int rc = check_point_blocks(P)) return rc;
    if (B > 0 && *G * C > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "output too large");
    *algo = resolve_algo_smooth_channels(*algo, op, n_out, grid, P, C);
    *need = smooth_workspace_bytes(op, *algo, n_out, grid, P);
    return *need == (size_t)-1 ? DPR_ERR_UNSUPPORTED_ALGO : DPR_OK;
}

template <typename T>
static int raster_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t C, T* out, const T* points,
                                       const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws,
                                       size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_channels(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need)) return rc;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !pw) return fail(DPR_ERR_INVALID_ARG, "point_weight is NULL with P > 0 (the channel form needs it)");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth splat with channels (algorithm %d) needs %zu workspace bytes, got %zu",
                    algo, need, ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    fill_background(st, out, G, B * C, bg);
    stage_mark(st);
    const int c = (int)C;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_channels_fwd_tiled<T, NI, NO>(st, grid, G, P, B, c, out, points, rot, trans, ow, pw,
                                                                  ws, ws_bytes)
                           : smooth_channels_fwd_atomic<T, NI, NO>(st, grid, G, P, B, c, out, points, rot, trans, ow,
                                                                   pw);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int pullback_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t* grid, int64_t P, int64_t B, int64_t C, const T* g,
                                         const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                                         T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws,
                                         size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_channels(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need))
        return rc;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    if (B == 0) return DPR_OK;  // (every output is empty)
    if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (!d_rot || !d_trans || !d_bg || !d_ow) return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !pw) return fail(DPR_ERR_INVALID_ARG, "point_weight is NULL with P > 0 (the channel form needs it)");
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    const int64_t planes = B * C;
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * n_out * n_in)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * n_out)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)planes));
    // ds_dbackground[b, c] = sum of plane b * C + c
    grid_sum(st, g, G, planes, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    if (P == 0) return DPR_OK;  // (the per-pose sums are 0, ds_dbackground is done)
    int64_t slices = 1;
    const int poses_per_slice = pose_slices(P, B, &slices);  // (the linear atomic pullback's: SUMMATION ORDER, note 1)
    const int c = (int)C;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = smooth_channels_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, c, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
            slices);
        stage_mark(st);
        return rc;
    });
}

static size_t workspace_smooth_channels_impl(int op, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t* grid, int64_t P, int64_t B, int64_t C) {
    int64_t G = 0;
    size_t need = 0;
    if (check_smooth_channels(op, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need)) return (size_t)-1;
    return need;
}

// ---------------------------------------------------------------- smooth sampling of C-channel images
// dpr_sample_smooth_channels_ex_* / dpr_sample_smooth_channels_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING,
// MULTI-CHANNEL"; kernels: dpr_sample_smooth_channels.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the
// fused kernel with C image atomics per cell; DPR_ALGO_TILED, the same kernel without them, then ds_dimage pose by
// pose from the tiled smooth channel forward -- one binning per pose for all C channels.
// AUTO: the forward is ATOMIC; the pullback is TILED where the smooth channel forward of one pose of the shape would
// be (resolve_algo_smooth_channels; the measured rows: profiles/sample_smooth_channels_probe.txt).
static int resolve_algo_sample_smooth_channels(int algo, int op, int n_out, const int64_t* grid, int64_t P,
                                               int64_t C) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op == DPR_OP_PULLBACK) return resolve_algo_smooth_channels(DPR_ALGO_AUTO, DPR_OP_RASTER, n_out, grid, P, C);
    return DPR_ALGO_ATOMIC;
}

// the host checks both entry points and the queries share: smooth sampling's, then C and the 64-bit offsets of the
// channel layouts; *G and the resolved *algo come back, *need: workspace (sample_smooth_workspace_bytes: the tiled
// smooth forward's for one pose, whatever B and C)
static int check_sample_smooth_channels(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                        int64_t P, int64_t B, int64_t C, int64_t* G, size_t* need) {
    if (int rc = check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (int rc = check_sample_smooth_op(op, flags)) return rc;
    if (C < 1 || C > kMaxChannels)
        return fail(DPR_ERR_INVALID_ARG, "channels C = %lld out of range [1, %d]", (long long)C, kMaxChannels);
    *algo = resolve_algo_sample_smooth_channels(*algo, op, n_out, grid, P, C);
    *need = sample_smooth_workspace_bytes(op, *algo, n_out, grid, P);
    if (*need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    if (int rc = check_sample_sizes(P, B, *G)) return rc;
    // 64-bit offsets: plane (c, b) starts at (b * C + c) * G, the values of (point p, pose b) at (b * P + p) * C
    if (B > 0 && (P > ((int64_t)1 << 62) / (B * C) || *G > ((int64_t)1 << 62) / (B * C)))
        return fail(DPR_ERR_INVALID_ARG, "P * C * B or the image (G * C * B) too large");
    return DPR_OK;
}

template <typename T>
static int sample_smooth_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t C, T* values, const T* image,
                                       const T* points, const T* rot, const T* trans, void* ws, size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth_channels(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need))
        return rc;
    if (P == 0 || B == 0) return DPR_OK;
    if (!values) return fail(DPR_ERR_INVALID_ARG, "values is NULL");
    if (!image) return fail(DPR_ERR_INVALID_ARG, "image is NULL");
    if (!points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (int rc = check_alignment<T>(ws, {values, image, points, rot, trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = sample_smooth_channels_fwd<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, (int)C, values, image, points, rot, trans, pps, slices);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int sample_smooth_channels_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                                const int64_t* grid, int64_t P, int64_t B, int64_t C, const T* dv,
                                                const T* image, const T* points, const T* rot, const T* trans,
                                                T* d_img, T* d_pts, T* d_rot, T* d_trans, void* ws, size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth_channels(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need))
        return rc;
    if (!d_img && !d_pts && !d_rot && !d_trans)
        return fail(DPR_ERR_INVALID_ARG, "smooth channel sampling pullback: every output is NULL");
    const bool tiled = algo == DPR_ALGO_TILED;
    if (tiled && d_img && P > 0 && B > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE,
                    "DPR_ALGO_TILED smooth channel sampling pullback needs %zu workspace bytes, got %zu", need,
                    ws ? ws_bytes : (size_t)0);
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && B > 0) {
        if (!dv) return fail(DPR_ERR_INVALID_ARG, "ds_dvalues is NULL");
        if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
        if ((d_pts || d_rot || d_trans) && !image)
            return fail(DPR_ERR_INVALID_ARG, "image is NULL (needed for ds_dpoints / ds_drotation / ds_dtranslation)");
    }
    if (int rc = check_alignment<T>(ws, {dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    if (d_rot) DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * n_out * n_in)));
    if (d_trans) DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * n_out)));
    if (d_img) DPR_HIP(zero_async(st, d_img, sizeof(T) * (size_t)(B * C * G)));
    if (d_pts && B == 0) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
    if (P == 0 || B == 0) return DPR_OK;
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    const int c = (int)C;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        if (int rc = sample_smooth_channels_bwd<T, NI, NO>(st, grid, G, P, B, c, dv, image, points, rot, trans,
                                                           tiled ? nullptr : d_img, d_pts, d_rot, d_trans, pps,
                                                           slices))
            return rc;
        stage_mark(st);
        if (tiled && d_img) {
            // the C planes of pose b (zeroed above): the single-pose tiled smooth channel forward of the weights
            // ds_dvalues[:, :, b] (P x C, contiguous), out_weight 1 -- what
            // dpr_raster_smooth_channels_ex_*(DPR_ALGO_TILED) returns for them
            for (int64_t b = 0; b < B; ++b)
                if (int rc = smooth_channels_fwd_tiled<T, NI, NO>(st, grid, G, P, 1, c, d_img + b * C * G, points,
                                                                  rot + b * (NO * NI), trans + b * NO, nullptr,
                                                                  dv + b * P * C, ws, ws_bytes))
                    return rc;
        }
        return DPR_OK;
    });
}

static size_t workspace_sample_smooth_channels_impl(int op, int algo, unsigned flags, int n_in, int n_out,
                                                    const int64_t* grid, int64_t P, int64_t B, int64_t C) {
    int64_t G = 0;
    size_t need = 0;
    if (check_sample_smooth_channels(op, &algo, flags, n_in, n_out, grid, P, B, C, &G, &need)) return (size_t)-1;
    return need;
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_smooth(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    int64_t G = 0;
    if (int rc = dpr::check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = dpr::check_smooth(op, 0u)) return rc;
    return dpr::resolve_algo_smooth(DPR_ALGO_AUTO, op, n_out, grid, P);
}

#define DPR_DEFINE_SMOOTH(SUF, T)                                                                              \
    size_t dpr_workspace_bytes_smooth_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,          \
                                               const int64_t* grid, int64_t P, int64_t B) {                    \
        return dpr::workspace_smooth_impl<T>(op, algo, flags, n_in, n_out, grid, P, B);                        \
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
    int64_t G = 0;
    if (int rc = dpr::check_smooth_dims(n_in, n_out)) return rc;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = dpr::check_sample_smooth_op(op, 0u)) return rc;
    return dpr::resolve_algo_sample_smooth(DPR_ALGO_AUTO, op, n_out, grid, P);
}

#define DPR_DEFINE_SAMPLE_SMOOTH(SUF, T)                                                                       \
    size_t dpr_workspace_bytes_sample_smooth_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,   \
                                                      const int64_t* grid, int64_t P, int64_t B) {             \
        return dpr::workspace_sample_smooth_impl<T>(op, algo, flags, n_in, n_out, grid, P, B);                 \
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
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_smooth_jvp(&algo, 0u, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SMOOTH_JVP(SUF, T)                                                                          \
    size_t dpr_workspace_bytes_smooth_jvp_ex_##SUF(int algo, unsigned flags, int n_in, int n_out,              \
                                                   const int64_t* grid, int64_t P, int64_t B, int64_t K) {     \
        return dpr::workspace_smooth_jvp_impl(algo, flags, n_in, n_out, grid, P, B, K);                        \
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
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_smooth_clouds(op, &algo, 0u, n_in, n_out, grid, P, B, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SMOOTH_CLOUDS(SUF, T)                                                                       \
    size_t dpr_workspace_bytes_smooth_clouds_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,   \
                                                      const int64_t* grid, int64_t P, int64_t B) {             \
        return dpr::workspace_smooth_clouds_impl(op, algo, flags, n_in, n_out, grid, P, B);                    \
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

int dpr_resolve_algo_smooth_channels(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                     int64_t C) {
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_smooth_channels(op, &algo, 0u, n_in, n_out, grid, P, B, C, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SMOOTH_CHANNELS(SUF, T)                                                                     \
    size_t dpr_workspace_bytes_smooth_channels_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out, \
                                                        const int64_t* grid, int64_t P, int64_t B, int64_t C) { \
        return dpr::workspace_smooth_channels_impl(op, algo, flags, n_in, n_out, grid, P, B, C);               \
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
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_sample_smooth_channels(op, &algo, 0u, n_in, n_out, grid, P, B, C, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SAMPLE_SMOOTH_CHANNELS(SUF, T)                                                              \
    size_t dpr_workspace_bytes_sample_smooth_channels_ex_##SUF(int op, int algo, unsigned flags, int n_in,     \
                                                               int n_out, const int64_t* grid, int64_t P,      \
                                                               int64_t B, int64_t C) {                         \
        return dpr::workspace_sample_smooth_channels_impl(op, algo, flags, n_in, n_out, grid, P, B, C);        \
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
