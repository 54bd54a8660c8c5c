// The smooth rigid-body entry points of libdpr -- splat, pullback, forward mode and sampling: what each family is, its
// AUTO rule, its extent and size bounds, and the C ABI (include/dpr.h, "SMOOTH SPLAT, RIGID BODIES", "SMOOTH SPLAT,
// RIGID BODIES, FORWARD MODE" and "SMOOTH SAMPLING, RIGID BODIES").  The checks, pointer checks, stream prologues and
// entry-point skeletons shared with the other smooth families: dpr_host_smooth.h (core: dpr_api.hip; kernels and their
// launches: dpr_smooth_bodies.hip, dpr_sample_smooth_bodies.hip).  Point p is seen in image b through pose
// b * K + body[p]: B images, B * K poses.
#include <hip/hip_runtime.h>

#include "dpr_host_smooth.h"

namespace dpr {

// ---------------------------------------------------------------- smooth splat of rigid bodies
// DPR_ALGO_ATOMIC: forward and pullback; DPR_ALGO_TILED: forward, the images binned in groups
// (DPR_FLAG_MAX_POSE_GROUP; the pullback forms none and refuses the flag).
constexpr SmoothFamily kSmoothBodies{"smooth rigid bodies", kTiledForward, /*residual_refusal*/ true,
                                     /*group_plan*/ true, kGroupRefusedOffTiledOp, /*has_body*/ true,
                                     /*needs_point_weight*/ false, /*pullback_slices_poses*/ true};

// AUTO (dpr_resolve_algo_smooth_bodies), from the shape alone.  The pullback is DPR_ALGO_ATOMIC.  The forward is
// DPR_ALGO_TILED where the default GROUP of images holds bg * P >= the constant below and the cloud holds at least
// kSmoothBodiesTiledMinPointsPerTile points per tile of the grid, DPR_ALGO_ATOMIC otherwise: the shape of
// dpr_resolve_algo_smooth_clouds' rule, because the tiled path pays its four launches per group here too.  K does not
// enter: TILED / ATOMIC move by less than 10 % from K = 1 to 64 and between a sorted and a shuffled cloud.  From this
// op's own rows (profiles/smooth_bodies_probe.txt, tests/golden/smooth_bodies_auto.json; fp32, ms TILED / ATOMIC):
//  - 3-D, 1e5 (the smooth clouds' constant, confirmed): 128^3, 1e4 x 4 images (bg * P = 4e4) 0.130 / 0.130 and
//    0.128 / 0.114, 3e4 x 4 (1.2e5) 0.155 / 0.214, 1e4 x 16 0.235 / 0.271, 1e6 x 4 0.35 / 4.4.
//  - 2-D, 1.6e5 (the smooth clouds' 4e5 lost this op's two lowest rows): 128^2, 1e4 x 16 (1.6e5) 0.121 / 0.144 --
//    1.19x, beyond the 1.15 margin -- 1e4 x 32 0.176 / 0.200, 3e4 x 16 0.192 / 0.266; 512^2, 3e4 x 16 0.203 / 0.269,
//    1e6 x 16 0.91 / 6.2.  TILED is ahead on every 2-D row measured; nothing was measured below 1.6e5.
//  - 4 points per tile (confirmed): 256^3 (16 384 tiles), 1e4 x 16 (0.6 per tile) 0.685 / 0.426, 3e4 x 4 (1.8)
//    0.309 / 0.244, 1e5 x 4 (6.1) 0.424 / 0.534; 128^3, 1e4 x 16 (4.9) 0.235 / 0.271.
constexpr int64_t kSmoothBodiesTiledMinWork3D = 100000;
constexpr int64_t kSmoothBodiesTiledMinWork2D = 160000;
constexpr int64_t kSmoothBodiesTiledMinPointsPerTile = 4;
static int resolve_algo_smooth_bodies(int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothBodiesTiledMinWork3D : kSmoothBodiesTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    return bg * P >= min_work && P / kSmoothBodiesTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED : DPR_ALGO_ATOMIC;
}

static SmoothCall check_smooth_bodies(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                      int64_t P, int64_t B, int64_t K) {
    return smooth_checks(
        kSmoothBodies, op, algo, flags, n_in, n_out, grid, P, B, [&] { return check_body_count(B, K); },
        [&](int64_t) { return check_point_blocks(P); },
        [&] { return resolve_algo_smooth_bodies(op, n_out, grid, P, B); });
}

template <typename T>
static int raster_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, int64_t K, T* out, const T* points, const int32_t* body,
                                     const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws,
                                     size_t ws_bytes) {
    const SmoothCall c = check_smooth_bodies(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, K);
    return smooth_splat_forward<T>(
        kSmoothBodies, c, stream, n_in, n_out, P, B, B, out, points, body, rot, trans, bg, ow, pw, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_bodies_fwd_tiled<T, NI, NO>(st, grid, c.G, P, B, (int)K, max_pose_group(flags), out,
                                                            points, body, rot, trans, ow, pw, ws, ws_bytes)
                       : smooth_bodies_fwd_atomic<T, NI, NO>(st, grid, c.G, P, B, (int)K, out, points, body, rot,
                                                             trans, ow, pw);
        });
}

template <typename T>
static int pullback_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t K, const T* g,
                                       const T* points, const int32_t* body, const T* rot, const T* trans,
                                       const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow,
                                       T* d_pw, void* ws) {
    const SmoothCall c = check_smooth_bodies(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B, K);
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    return smooth_splat_pullback<T>(
        kSmoothBodies, c, stream, flags, n_in, n_out, P, B, B, B * K, g, points, body, rot, trans, ow, pw, d_pts,
        d_rot, d_trans, d_bg, d_ow, d_pw, ws,
        [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return smooth_bodies_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)K, g, points, body, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw,
                poses_per_slice, slices);
        });
}

// ---------------------------------------------------------------- forward mode
// DPR_ALGO_ATOMIC and DPR_ALGO_TILED; DPR_FLAG_MAX_POSE_GROUP sizes the groups of a TILED call.
constexpr SmoothFamily kSmoothBodiesJvp{"smooth rigid-body JVP", kTiledOnlyOp, /*residual_refusal*/ false,
                                        /*group_plan*/ true, kGroupIgnored, /*has_body*/ true,
                                        /*needs_point_weight*/ false, /*pullback_slices_poses*/ false};

// AUTO (dpr_resolve_algo_smooth_bodies_jvp), from the shape and V alone: the forward's rule -- DPR_ALGO_TILED where the
// default GROUP holds enough work and the cloud at least 4 points per tile -- with the group's work counted as
// bg * P * V^2.  The rule started as the forward's with bg * P * V (what dpr_resolve_algo_smooth_jvp does with P * K);
// this op's own rows (profiles/smooth_bodies_jvp_probe.txt, tests/golden/smooth_bodies_jvp_auto.json; fp32, K = 4,
// ms ATOMIC / TILED) leave no constant for that product: on 128^2 1000 x 4 images at V = 12 (bg * P * V = 4.8e4) is
// 0.111 / 0.087 -- TILED 1.28x ahead -- and 1e4 x 8 at V = 1 (8e4) 0.095 / 0.122 -- ATOMIC 1.28x ahead; on 64^3 1100 x 2 at
// V = 12 (2.6e4) 0.205 / 0.122 against 1e4 x 4 at V = 1 (4e4, 128^3) 0.117 / 0.147.  The binning is paid once per group
// whatever V and costs about what one tangent's atomics cost, so the bg * P from which TILED pays falls faster than
// 1 / V: at V = 12 TILED is ahead on every row measured with 4 points per tile (down to bg * P = 2200), at V = 1 from about the forward's
// constants on.  V^2 puts both on one side of one constant each:
//  - 2-D, 1.6e5 (the forward's, confirmed): V = 1, 128^2, 1e4 x 12 (1.2e5) 0.111 / 0.126, 1e4 x 16 (1.6e5) 0.126 / 0.132 --
//    1.04x behind --, 3e4 x 16 0.255 / 0.204.
//  - 3-D, 9.6e4 (the forward's 1e5 lost this op's row 64^3, 24 000 x 4 at V = 1: 0.178 / 0.133, 1.34x): below it 1e4 x 4
//    (4e4) 0.108 / 0.113 on 64^3 and 0.117 / 0.147 on 128^3.
//  - 4 points per tile (confirmed): 256^3, 1e4 x 16 (0.6 per tile) 0.44 / 0.80 and 4.39 / 7.65 at V = 12, 3e4 x 4 (1.8)
//    0.25 / 0.36 and 2.17 / 3.15, 1e5 x 4 (6.1) 0.53 / 0.49 and 5.64 / 4.06.
// Only V = 1 and V = 12 were measured: between them the square is an interpolation.
constexpr int64_t kSmoothBodiesJvpTiledMinWork3D = 96000;
constexpr int64_t kSmoothBodiesJvpTiledMinWork2D = 160000;
constexpr int64_t kSmoothBodiesJvpTiledMinPointsPerTile = 4;
static int resolve_algo_smooth_bodies_jvp(int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t V) {
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothBodiesJvpTiledMinWork3D : kSmoothBodiesJvpTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    // (bg * P <= 2^24 for bg > 1, P < 2^32 for bg = 1, V <= 16: the product stays inside 64 bits)
    return bg * P * V * V >= min_work && P / kSmoothBodiesJvpTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED
                                                                                          : DPR_ALGO_ATOMIC;
}

static SmoothCall check_smooth_bodies_jvp(int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                          int64_t P, int64_t B, int64_t K, int64_t V) {
    return smooth_checks(
        kSmoothBodiesJvp, DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B,
        [&] {
            if (int rc = check_body_count(B, K)) return rc;
            return check_jvp(V, 0u);  // (V in 1 .. kMaxTangents)
        },
        [&](int64_t G) {
            if (int rc = check_sample_sizes(P, B, G)) return rc;
            return check_plane_offsets(G, V, B);
        },
        [&] { return resolve_algo_smooth_bodies_jvp(n_out, grid, P, B, V); });
}

template <typename T>
static int raster_smooth_bodies_jvp_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t* grid, int64_t P, int64_t B, int64_t K, int64_t V, T* out_dot,
                                         const T* points, const int32_t* body, const T* rot, const T* trans,
                                         const T* ow, const T* pw, JvpTangents<T> tan, const T* bg_dot, void* ws,
                                         size_t ws_bytes) {
    const SmoothCall c = check_smooth_bodies_jvp(algo, flags, n_in, n_out, grid, P, B, K, V);
    return smooth_jvp_forward<T>(
        kSmoothBodiesJvp, c, stream, n_in, n_out, P, B, V, out_dot, points, body, rot, trans, ow, pw, tan, bg_dot, ws,
        ws_bytes, [&](hipStream_t st, auto ni, auto no) {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            return c.algo == DPR_ALGO_TILED
                       ? smooth_bodies_jvp_tiled<T, NI, NO>(st, grid, c.G, P, B, (int)K, (int)V,
                                                            max_pose_group(flags), out_dot, points, body, rot, trans,
                                                            ow, pw, tan, ws, ws_bytes)
                       : smooth_bodies_jvp_atomic<T, NI, NO>(st, grid, c.G, P, B, (int)K, (int)V, out_dot, points,
                                                             body, rot, trans, ow, pw, tan);
        });
}

// ---------------------------------------------------------------- smooth sampling at the points of rigid bodies
// dpr_sample_smooth_bodies_ex_* / dpr_sample_smooth_bodies_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING, RIGID
// BODIES"; kernels: dpr_sample_smooth_bodies.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the fused
// point kernel with image atomics; DPR_ALGO_TILED, the same kernel without them, then ds_dimage group by group of
// images through the binning of the tiled smooth rigid-body forward.
// AUTO: the forward is ATOMIC; the pullback is TILED exactly where the smooth rigid-body forward of the shape would
// be (resolve_algo_smooth_bodies above; dpr_resolve_algo_sample_smooth's precedent).
static int resolve_algo_sample_smooth_bodies(int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (op != DPR_OP_PULLBACK) return DPR_ALGO_ATOMIC;
    return resolve_algo_smooth_bodies(DPR_OP_RASTER, n_out, grid, P, B);
}

// (DPR_FLAG_MAX_POSE_GROUP sizes the groups of a TILED pullback; every other call refuses it)
constexpr SmoothFamily kSmoothBodySampling{"smooth rigid-body sampling", kTiledPullback, /*residual_refusal*/ false,
                                           /*group_plan*/ true, kGroupRefusedOffTiled, /*has_body*/ true,
                                           /*needs_point_weight*/ false, /*pullback_slices_poses*/ false};

static SmoothCall check_sample_smooth_bodies(int op, int algo, unsigned flags, int n_in, int n_out,
                                             const int64_t* grid, int64_t P, int64_t B, int64_t K) {
    return smooth_checks(
        kSmoothBodySampling, op, algo, flags, n_in, n_out, grid, P, B, [&] { return check_body_count(B, K); },
        [&](int64_t G) { return check_sample_sizes(P, B, G); },
        [&] { return resolve_algo_sample_smooth_bodies(op, n_out, grid, P, B); });
}

template <typename T>
static int sample_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, int64_t K, T* values, const T* image, const T* points,
                                     const int32_t* body, const T* rot, const T* trans, void* ws) {
    const SmoothCall c = check_sample_smooth_bodies(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, K);
    return smooth_sample_forward<T>(
        kSmoothBodySampling, c, stream, n_in, n_out, P, B, values, image, points, body, rot, trans, ws,
        [&](hipStream_t st, auto ni, auto no, int poses_per_slice, int64_t slices) {
            return sample_smooth_bodies_fwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)K, values, image, points, body, rot, trans, poses_per_slice, slices);
        });
}

template <typename T>
static int sample_smooth_bodies_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                              const int64_t* grid, int64_t P, int64_t B, int64_t K, const T* dv,
                                              const T* image, const T* points, const int32_t* body, const T* rot,
                                              const T* trans, T* d_img, T* d_pts, T* d_rot, T* d_trans, void* ws,
                                              size_t ws_bytes) {
    const SmoothCall c = check_sample_smooth_bodies(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B, K);
    return smooth_sample_pullback<T>(
        kSmoothBodySampling, c, stream, n_in, n_out, P, B, B, B * K, dv, image, points, body, rot, trans, d_img, d_pts,
        d_rot, d_trans, ws, ws_bytes,
        [&](hipStream_t st, auto ni, auto no, T* d_img_atomic, int poses_per_slice, int64_t slices) {
            return sample_smooth_bodies_bwd<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)K, dv, image, points, body, rot, trans, d_img_atomic, d_pts, d_rot, d_trans,
                poses_per_slice, slices);
        },
        [&](hipStream_t st, auto ni, auto no) {
            return sample_smooth_bodies_image_tiled<T, decltype(ni)::value, decltype(no)::value>(
                st, grid, c.G, P, B, (int)K, max_pose_group(flags), d_img, dv, points, body, rot, trans, ws, ws_bytes);
        });
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_sample_smooth_bodies(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                          int64_t K) {
    return dpr::resolver_value(dpr::check_sample_smooth_bodies(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, K));
}

#define DPR_DEFINE_SAMPLE_SMOOTH_BODIES(SUF, T)                                                                     \
    size_t dpr_workspace_bytes_sample_smooth_bodies_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out, \
                                                             const int64_t* grid, int64_t P, int64_t B,             \
                                                             int64_t K) {                                           \
        return dpr::query_value(dpr::check_sample_smooth_bodies(op, algo, flags, n_in, n_out, grid, P, B, K));      \
    }                                                                                                               \
    int dpr_sample_smooth_bodies_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,              \
                                          const int64_t* grid, int64_t P, int64_t B, int64_t K, T* values,          \
                                          const T* image, const T* points, const void* body, const T* rotation,     \
                                          const T* translation, void* workspace, size_t workspace_bytes) {          \
        (void)workspace_bytes;                                                                                      \
        return dpr::sample_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, values, image,    \
                                                 points, (const int32_t*)body, rotation, translation, workspace);   \
    }                                                                                                               \
    int dpr_sample_smooth_bodies_pullback_ex_##SUF(                                                                 \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,     \
        int64_t K, const T* ds_dvalues, const T* image, const T* points, const void* body, const T* rotation,       \
        const T* translation, T* ds_dimage, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, void* workspace,    \
        size_t workspace_bytes) {                                                                                   \
        return dpr::sample_smooth_bodies_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K,          \
                                                          ds_dvalues, image, points, (const int32_t*)body,          \
                                                          rotation, translation, ds_dimage, ds_dpoints,             \
                                                          ds_drotation, ds_dtranslation, workspace,                 \
                                                          workspace_bytes);                                         \
    }
DPR_DEFINE_SAMPLE_SMOOTH_BODIES(f32, float)
DPR_DEFINE_SAMPLE_SMOOTH_BODIES(f64, double)
#undef DPR_DEFINE_SAMPLE_SMOOTH_BODIES

int dpr_resolve_algo_smooth_bodies(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                   int64_t K) {
    return dpr::resolver_value(dpr::check_smooth_bodies(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, K));
}

#define DPR_DEFINE_SMOOTH_BODIES(SUF, T)                                                                          \
    size_t dpr_workspace_bytes_smooth_bodies_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,      \
                                                      const int64_t* grid, int64_t P, int64_t B, int64_t K) {     \
        return dpr::query_value(dpr::check_smooth_bodies(op, algo, flags, n_in, n_out, grid, P, B, K));           \
    }                                                                                                             \
    int dpr_raster_smooth_bodies_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,            \
                                          const int64_t* grid, int64_t P, int64_t B, int64_t K, T* out,           \
                                          const T* points, const void* body, const T* rotation,                   \
                                          const T* translation, const T* background, const T* out_weight,         \
                                          const T* point_weight, void* workspace, size_t workspace_bytes) {       \
        return dpr::raster_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, out, points,    \
                                                 (const int32_t*)body, rotation, translation, background,         \
                                                 out_weight, point_weight, workspace, workspace_bytes);           \
    }                                                                                                             \
    int dpr_raster_pullback_smooth_bodies_ex_##SUF(                                                               \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,   \
        int64_t K, const T* ds_dout, const T* points, const void* body, const T* rotation, const T* translation,  \
        const T* out_weight, const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation,           \
        T* ds_dbackground, T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {     \
        (void)workspace_bytes;                                                                                    \
        return dpr::pullback_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, ds_dout,      \
                                                   points, (const int32_t*)body, rotation, translation,           \
                                                   out_weight, point_weight, ds_dpoints, ds_drotation,            \
                                                   ds_dtranslation, ds_dbackground, ds_dout_weight,               \
                                                   ds_dpoint_weight, workspace);                                  \
    }
DPR_DEFINE_SMOOTH_BODIES(f32, float)
DPR_DEFINE_SMOOTH_BODIES(f64, double)
#undef DPR_DEFINE_SMOOTH_BODIES

int dpr_resolve_algo_smooth_bodies_jvp(int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t K,
                                       int64_t V) {
    return dpr::resolver_value(dpr::check_smooth_bodies_jvp(DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, K, V));
}

#define DPR_DEFINE_SMOOTH_BODIES_JVP(SUF, T)                                                                      \
    size_t dpr_workspace_bytes_smooth_bodies_jvp_ex_##SUF(int algo, unsigned flags, int n_in, int n_out,          \
                                                          const int64_t* grid, int64_t P, int64_t B, int64_t K,   \
                                                          int64_t V) {                                            \
        return dpr::query_value(dpr::check_smooth_bodies_jvp(algo, flags, n_in, n_out, grid, P, B, K, V));        \
    }                                                                                                             \
    int dpr_raster_smooth_bodies_jvp_ex_##SUF(                                                                    \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,   \
        int64_t K, int64_t V, T* out_dot, const T* points, const void* body, const T* rotation,                   \
        const T* translation, const T* out_weight, const T* point_weight, const T* points_dot,                    \
        const T* rotation_dot, const T* translation_dot, const T* background_dot, const T* out_weight_dot,        \
        const T* point_weight_dot, void* workspace, size_t workspace_bytes) {                                     \
        return dpr::raster_smooth_bodies_jvp_impl<T>(                                                             \
            stream, algo, flags, n_in, n_out, grid, P, B, K, V, out_dot, points, (const int32_t*)body, rotation,  \
            translation, out_weight, point_weight,                                                                \
            dpr::JvpTangents<T>{points_dot, rotation_dot, translation_dot, out_weight_dot, point_weight_dot},     \
            background_dot, workspace, workspace_bytes);                                                          \
    }
DPR_DEFINE_SMOOTH_BODIES_JVP(f32, float)
DPR_DEFINE_SMOOTH_BODIES_JVP(f64, double)
#undef DPR_DEFINE_SMOOTH_BODIES_JVP

}  // extern "C"
